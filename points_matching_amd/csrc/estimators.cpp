// estimators.cpp — the C-ABI entry points of the robust model families of include/pm.h that share one call shape:
// the homography (RANSAC-H, ransac_h_fused.hip, refined by homography_refine.hip), the affine / similarity model
// (RANSAC-A, ransac_a_fused.hip, refitted by affine_refine.hip), the calibrated relative pose (RANSAC-E,
// essential_solve.hip + ransac_e_fused.hip, followed by recover_pose.hip and, on request, pose_refine.hip), the
// absolute pose (RANSAC-PnP, pnp_solve.hip + ransac_p_fused.hip, refined by pnp_refine.hip) and the 3-D to 3-D
// alignment (rigid / similarity transforms, align3d_solve.hip + ransac_align3d_fused.hip, refitted by
// align3d_refine.hip); also the refinement of the fundamental matrix (fundamental_refine.hip; its RANSAC is the one-launch kernel of ransac_fused.hip, whose other entry
// points live in ransac.hip) and of a relative pose alone (pose_refine.hip).  Those files hold the kernels and one enqueue
// each.
// Here: one description per family (Family), every argument check once, and one driver per call shape — run_host for
// the host-pointer forms (upload, RANSAC and / or the second step on one stream, one readback into pinned memory, one
// synchronisation), run_dev / refine_dev for the device forms.  The families differ in data and in which launch is
// enqueued (three switches below); the extern "C" functions at the end are one call each.
#include <cmath>

#include "affine_core.hpp"
#include "align3d_core.hpp"
#include "ransac_internal.hpp"

namespace pm_ransac {
namespace {

enum Id { H, A, E, P, F, R, X };    // R: a relative pose (R, t) to refine, no RANSAC of its own; X: 3-D to 3-D alignment

// One model family.  A sample yields `ids` candidate models (model ids ids * h + j); the minimal solvers of E and P write
// them `stride` doubles apart with a non-zero flag at offset `flag`, and so does the one of X for its one model.  The
// second step is LM with max_iters (H, P), the closed-form refit (A, X) or pose recovery with dist (E), which a third step may follow: LM on the recovered pose.
struct Family {
    Id id;
    const char* name;           // in messages
    int words;                  // doubles of a model: H 9, A 6, E 9, P 12 (R, then t), X 13 (R, t, s)
    int min_pts;
    int dim1, dim2;             // floats per point of the first and the second array (P: world points; X: 3 and 3)
    int ids, stride, flag;
    int error_kind;
    const char* unit;           // what RANSAC draws, in messages
    const char* null_model;     // messages of the null checks
    const char* null_cands;
    int model;                  // A: PM_AFFINE_FULL | PM_AFFINE_PARTIAL; X: PM_ALIGN3D_RIGID | PM_ALIGN3D_SIMILARITY
    int max_iters;              // H, P, F, R; E: of the third step
    double dist;                // E
    bool third;                 // E: refine the recovered pose
    bool lm() const { return id == H || id == P || id == F || id == R || third; }
    bool camera() const { return id == E || id == P || id == R; }
    bool pose() const { return id == E; }       // the second step maps the model to (R, t, mask, points), not to a model
};

Family homography(int max_iters)
{
    return Family{H, "H", 9, 4, 2, 2, 1, 0, 0, PM_ERR_REPROJ, "hypotheses", "null H", nullptr, 0, max_iters, 0.0};
}
Family affine(int model)
{
    using namespace pm_affine;
    const int k = model == PM_AFFINE_FULL ? Traits<FULL>::MIN_PTS : Traits<PARTIAL>::MIN_PTS;
    return Family{A, "A", 6, k, 2, 2, 1, 0, 0, PM_ERR_REPROJ, "hypotheses", "null A", nullptr, model, 0, 0.0};
}
Family essential(double dist, bool third = false, int max_iters = 0)
{
    return Family{E, "E", 9, 5, 2, 2, 10, 10, 9, PM_ERR_SAMPSON, "samples", "null E", "null E or counts", 0, max_iters, dist, third};
}
Family fundamental(int max_iters)
{
    return Family{F, "F", 9, 8, 2, 2, 1, 0, 0, PM_ERR_SAMPSON, "hypotheses", "null F", nullptr, 0, max_iters, 0.0};
}
Family relpose(int max_iters)
{
    return Family{R, "pose", 12, 5, 2, 2, 1, 0, 0, PM_ERR_SAMPSON, "samples", "null R or t", nullptr, 0, max_iters, 0.0};
}
Family pnp(int max_iters)
{
    return Family{P, "pose", 12, 4, 3, 2, 4, 20, 12, PM_ERR_REPROJ, "samples", "null R or t", "null Rt or counts", 0,
                  max_iters, 0.0};
}
Family align3d(int model)
{
    using namespace pm_align3d;
    return Family{X, "T", WORDS, 3, 3, 3, 1, SLOT_DOUBLES, FLAG, PM_ERR_REPROJ, "samples", "null T", nullptr, model, 0, 0.0};
}

// What a call runs: RANSAC, the second step (on RANSAC's winner, or on the caller's model), or both in that order;
// CANDIDATES: every candidate of p's one sample, each scored alone.
enum Steps { RANSAC = 1, SECOND = 2, CANDIDATES = 4 };

// Sample ids [begin, end) give model ids [ids * begin, ids * end), which a key and a single launch must hold
int check_range(const pm_ransac_params* p, int ids)
{
    if (!(p->hyp_begin >= 0 && p->hyp_end > p->hyp_begin && p->hyp_end <= 0x100000000LL / ids)) {
        pm::set_error("check_range: sample ids must satisfy 0 <= begin < end and %d * end <= 2^32 (%d model id(s) each)",
                      ids, ids);
        return PM_E_INVALID;
    }
    if (!(ids * (p->hyp_end - p->hyp_begin) <= 0x7FFFFFFFLL)) {
        pm::set_error("check_range: a single launch takes at most (2^31 - 1) / %d samples: split the range", ids);
        return PM_E_INVALID;
    }
    return PM_OK;
}

int check_K(const pm_camera* K)
{
    PM_REQUIRE(K != nullptr, PM_E_INVALID, "K is null");
    const bool fin = std::isfinite(K->fx) && std::isfinite(K->fy) && std::isfinite(K->cx) && std::isfinite(K->cy);
    PM_REQUIRE(fin && K->fx > 0.0 && K->fy > 0.0, PM_E_INVALID, "K needs finite values and fx, fy > 0");
    return PM_OK;
}

// The family's own checks, in the order every entry point runs them: model (A, X); params: null, range, error_kind,
// thresh_px (P, X); K, and for E the threshold normalised by it (S31, fp32); a null input model (no RANSAC); the second
// step's max_iters (H, P) or dist (E).  *thr: the threshold the scorer takes.
int check_args(const Family& f, int steps, const pm_ransac_params* p, const pm_camera* K, const double* model_in,
               float* thr)
{
    const bool ransac = steps & (RANSAC | CANDIDATES);
    if (f.id == A)
        PM_REQUIRE(f.model == PM_AFFINE_FULL || f.model == PM_AFFINE_PARTIAL, PM_E_INVALID,
                   "model must be PM_AFFINE_FULL or PM_AFFINE_PARTIAL");
    if (f.id == X)
        PM_REQUIRE(f.model == PM_ALIGN3D_RIGID || f.model == PM_ALIGN3D_SIMILARITY, PM_E_INVALID,
                   "model must be PM_ALIGN3D_RIGID or PM_ALIGN3D_SIMILARITY");
    if (ransac) {
        PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
        const int rc = check_range(p, f.ids);
        if (rc != PM_OK) return rc;
        if (f.id == F)
            PM_REQUIRE(p->error_kind == PM_ERR_SAMPSON || p->error_kind == PM_ERR_SYM_EPIPOLAR, PM_E_INVALID,
                       "unknown error_kind");
        else
            PM_REQUIRE(p->error_kind == f.error_kind, PM_E_INVALID,
                       f.error_kind == PM_ERR_SAMPSON ? "error_kind must be PM_ERR_SAMPSON" : "error_kind must be PM_ERR_REPROJ");
        if (f.id == P || f.id == X)
            PM_REQUIRE(p->thresh_px > 0.0f && std::isfinite(p->thresh_px), PM_E_INVALID, "thresh_px must be finite and > 0");
    }
    *thr = ransac ? p->thresh_px : 1.0f;
    if (f.camera()) {
        const int rc = check_K(K);
        if (rc != PM_OK) return rc;
    }
    if (f.id == E) {
        *thr = static_cast<float>(static_cast<double>(*thr) / (0.5 * (K->fx + K->fy)));
        PM_REQUIRE(*thr > 0.0f && std::isfinite(*thr), PM_E_INVALID, "the normalised threshold must be finite and > 0");
    }
    if (!ransac) PM_REQUIRE(model_in != nullptr, PM_E_INVALID, f.null_model);
    if ((steps & SECOND) && f.lm())
        PM_REQUIRE(f.max_iters >= 0 && f.max_iters <= 100, PM_E_INVALID, "max_iters must lie in [0, 100]");
    if ((steps & SECOND) && f.id == E) PM_REQUIRE(f.dist > 0.0, PM_E_INVALID, "dist must be > 0");
    return PM_OK;
}

// The scorer's parameters: model ids [ids * begin, ids * end) and the threshold check_args gave
pm_ransac_params model_ids(const Family& f, const pm_ransac_params* p, float thr)
{
    pm_ransac_params q = *p;
    q.hyp_begin = f.ids * p->hyp_begin;
    q.hyp_end = f.ids * p->hyp_end;
    q.thresh_px = thr;
    return q;
}

// Arena bytes of a RANSAC run over a view of cap_total points: what enqueue_solve carves (E: the normalised copy and its
// count; E, P, X: the candidates), the scorer's workgroup slots, 1 KiB of alignment slack.
size_t scratch_bytes(const pm_ctx* ctx, const Family& f, long long cap_total, const pm_ransac_params* p, float thr)
{
    const pm_ransac_params q = model_ids(f, p, thr);
    const size_t nh = static_cast<size_t>(p->hyp_end - p->hyp_begin);
    size_t solve = f.stride > 0 ? pm::align_up(sizeof(double) * f.ids * f.stride * nh, 256) : 0;
    if (f.id == E) solve += 2 * pm::align_up(sizeof(float) * 2 * static_cast<size_t>(cap_total), 256) + 256;
    return solve + fused_scratch_bytes(ctx, &q) + 1024;
}

// The minimal solver of samples [hyp_begin, hyp_end) of p, where it is a launch of its own (E, P, X; H and A solve inside
// their scorer): *d_cand receives the candidates, ids * stride doubles per sample, and *vs the view the scorer reads
// (E: the copy normalised by K).  Carves from the arena.
int enqueue_solve(pm_ctx* ctx, const Family& f, const pm_points_view& v, const pm_camera* K, const pm_ransac_params* p,
                  double** d_cand, pm_points_view* vs)
{
    const size_t cand_bytes = sizeof(double) * f.ids * f.stride * static_cast<size_t>(p->hyp_end - p->hyp_begin);
    *d_cand = nullptr;
    *vs = v;
    switch (f.id) {
    case H:
    case A:
    case F:
    case R:
        return PM_OK;
    case E: {
        const long long cap_total = static_cast<long long>(v.parts) * v.cap;
        float* xyn = static_cast<float*>(pm::arena_take(ctx, sizeof(float) * 4 * static_cast<size_t>(cap_total)));
        int* dn = static_cast<int*>(pm::arena_take(ctx, sizeof(int)));
        *d_cand = static_cast<double*>(pm::arena_take(ctx, cand_bytes));
        PM_REQUIRE(xyn && dn && *d_cand, PM_E_NOMEM, "scratch arena too small");
        *vs = pm_points_view{xyn, xyn + 2 * cap_total, dn, 1, static_cast<int32_t>(cap_total), 0, 1, 0};
        return essential_solve_enqueue(ctx, v, *K, p, xyn, dn, *d_cand);
    }
    case P:
        *d_cand = static_cast<double*>(pm::arena_take(ctx, cand_bytes));
        PM_REQUIRE(*d_cand, PM_E_NOMEM, "scratch arena too small");
        return pnp_solve_enqueue(ctx, v, *K, p, *d_cand);
    case X:
        *d_cand = static_cast<double*>(pm::arena_take(ctx, cand_bytes));
        PM_REQUIRE(*d_cand, PM_E_NOMEM, "scratch arena too small");
        return align3d_solve_enqueue(ctx, f.model, v, p, *d_cand);
    }
    return PM_E_INVALID;
}

// The one-launch scorer over model ids [q->hyp_begin, q->hyp_end), d_cand at the first of them
int enqueue_score(pm_ctx* ctx, const Family& f, const pm_points_view& vs, const pm_ransac_params* q, const double* d_cand,
                  unsigned long long* d_key, double* d_model, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    switch (f.id) {
    case H: return ransac_h_enqueue(ctx, vs, q, d_key, d_model, d_mask, mask_len, d_ninl);
    case A: return ransac_a_enqueue(ctx, f.model, vs, q, d_key, d_model, d_mask, mask_len, d_ninl);
    case E: return ransac_e_enqueue(ctx, vs, q, d_cand, d_key, d_model, d_mask, mask_len, d_ninl);
    case P: return ransac_p_enqueue(ctx, vs, q, d_cand, d_key, d_model, d_mask, mask_len, d_ninl);
    case F: return fused_launch(ctx, vs, q, 0, nullptr, d_key, d_model, d_mask, mask_len, d_ninl, nullptr);
    case X: return ransac_align3d_enqueue(ctx, vs, q, d_cand, d_key, d_model, d_mask, mask_len, d_ninl);
    case R: break;
    }
    return PM_E_INVALID;
}

// RANSAC on ctx->stream, the arena holding scratch_bytes() more
int enqueue_ransac(pm_ctx* ctx, const Family& f, const pm_points_view& v, const pm_camera* K, const pm_ransac_params* p,
                   float thr, unsigned long long* d_key, double* d_model, uint8_t* d_mask, int mask_len, int* d_ninl)
{
    double* d_cand = nullptr;
    pm_points_view vs{};
    const int rc = enqueue_solve(ctx, f, v, K, p, &d_cand, &vs);
    if (rc != PM_OK) return rc;
    const pm_ransac_params q = model_ids(f, p, thr);
    return enqueue_score(ctx, f, vs, &q, d_cand, d_key, d_model, d_mask, mask_len, d_ninl);
}

// The second step of the families where it maps a model to a model (pose recovery: recover_pose_enqueue).  d_E: R only,
// the E of the refined pose (may be null)
int enqueue_refine(pm_ctx* ctx, const Family& f, const pm_points_view& v, const pm_camera* K, const uint8_t* d_mask,
                   const double* d_in, double* d_out, pm_h_refine_info* d_info, double* d_E = nullptr)
{
    switch (f.id) {
    case H: return homography_refine_enqueue(ctx, v, d_mask, d_in, f.max_iters, d_out, d_info);
    case A: return affine_refine_enqueue(ctx, f.model, v, d_mask, d_in, d_out, d_info);
    case P: return pnp_refine_enqueue(ctx, v, *K, d_mask, d_in, f.max_iters, d_out, d_info);
    case F: return fundamental_refine_enqueue(ctx, v, d_mask, d_in, f.max_iters, d_out, d_info);
    case R: return pose_refine_enqueue(ctx, v, *K, d_mask, d_in, f.max_iters, d_out, d_E, d_info);
    case X: return align3d_refine_enqueue(ctx, f.model, v, d_mask, d_in, d_out, d_info);
    case E: break;
    }
    return PM_E_INVALID;
}

// The small results of a host-pointer call: one block on the device and its mirror in pinned memory (mask and points4
// follow the pinned one), read back as a whole, so each family's block holds what that family writes and no more:
//   key, count, n_good | info (E: R, t of the pose) | model | E, P: the candidates' keys, the candidates of the sample
//   | R, and E with a third step: the E of the refined pose | E with a third step: its info
struct Results {
    unsigned long long* key;
    int32_t *count, *n_good;
    pm_h_refine_info* info;     // H, A, P, X
    double* pose;               // E: R (9), t (3)
    double* model;
    unsigned long long* keys;
    double* cand;
    double* E_ref;
    pm_h_refine_info* info3;
};

// H 120, A 96, E 1064 (1168 with a third step), P 816, F 120, R 216, X 152
size_t results_bytes(const Family& f)
{
    const size_t second = f.pose() ? sizeof(double) * 12 : sizeof(pm_h_refine_info);
    return 16 + second + sizeof(double) * f.words + (f.ids > 1 ? sizeof(double) * f.ids * (1 + f.stride) : 0) +
           (f.id == R || f.third ? sizeof(double) * 9 : 0) + (f.third ? sizeof(pm_h_refine_info) : 0);
}

Results results_at(const Family& f, void* base)
{
    Results r;
    r.key = static_cast<unsigned long long*>(base);
    r.count = reinterpret_cast<int32_t*>(r.key + 1);
    r.n_good = r.count + 1;
    r.info = reinterpret_cast<pm_h_refine_info*>(r.key + 2);
    r.pose = reinterpret_cast<double*>(r.key + 2);
    r.model = f.pose() ? r.pose + 12 : reinterpret_cast<double*>(r.info + 1);
    r.keys = reinterpret_cast<unsigned long long*>(r.model + f.words);
    r.cand = reinterpret_cast<double*>(r.keys + f.ids);
    r.E_ref = f.ids > 1 ? r.cand + f.ids * f.stride : r.model + f.words;
    r.info3 = reinterpret_cast<pm_h_refine_info*>(r.E_ref + 9);
    return r;
}

// Every candidate of p's one sample scored alone (model ids [ids * hyp + j, ids * hyp + j + 1): its key holds its count),
// then the candidates copied next to the keys
int enqueue_candidates(pm_ctx* ctx, const Family& f, const pm_points_view& v, const pm_camera* K,
                       const pm_ransac_params* p, float thr, const Results& d, uint8_t* d_mask)
{
    double* d_cand = nullptr;
    pm_points_view vs{};
    int rc = enqueue_solve(ctx, f, v, K, p, &d_cand, &vs);
    if (rc != PM_OK) return rc;
    for (int j = 0; j < f.ids; ++j) {
        pm_ransac_params q = model_ids(f, p, thr);
        q.hyp_begin += j;
        q.hyp_end = q.hyp_begin + 1;
        rc = enqueue_score(ctx, f, vs, &q, d_cand + f.stride * j, &d.keys[j], nullptr, d_mask, 0, nullptr);
        if (rc != PM_OK) return rc;
    }
    PM_HIP_CHECK(hipMemcpyAsync(d.cand, d_cand, sizeof(double) * f.ids * f.stride, hipMemcpyDeviceToDevice, ctx->stream));
    return PM_OK;
}

// The host outputs of a call; any may be null except where a check says otherwise
struct HostOut {
    double* model;              // the first 9 words of the model (A: all 6)
    uint8_t* mask;              // n bytes
    int* n_inliers;
    uint64_t* best_key;
    pm_h_refine_info* info;
    double* tail;               // the rest of the model (P: t; X: t, s)
    double *R, *t;              // pose recovery
    int* n_good;
    float* points4;             // 4 n
    double* cands;              // CANDIDATES: ids * words
    int32_t* counts;            // CANDIDATES: ids
    int* n_models;
    double* E_ref;              // R: the E of the refined pose
};

void put_model(const Family& f, const HostOut& out, const double* src)
{
    const int w = f.words < 9 ? f.words : 9;
    if (out.model) memcpy(out.model, src, sizeof(double) * w);
    if (out.tail) memcpy(out.tail, src + w, sizeof(double) * (f.words - w));
}

// What a refused call leaves in its outputs: zeros (counts: -1; info: status 2), or with no RANSAC the input model `in`
// passed through and info status 1
void reset_outputs(const Family& f, bool ransac, int n, const double* in, const HostOut& out)
{
    put_model(f, out, in);
    if (out.mask && n > 0) memset(out.mask, 0, static_cast<size_t>(n));
    if (out.n_inliers) *out.n_inliers = 0;
    if (out.best_key) *out.best_key = 0;
    if (out.info) *out.info = pm_h_refine_info{0.0, 0.0, 0, 0, ransac ? 2 : 1, 0};
    if (out.R) memset(out.R, 0, sizeof(double) * 9);
    if (out.t) memset(out.t, 0, sizeof(double) * 3);
    if (out.n_good) *out.n_good = 0;
    if (out.points4 && n > 0) memset(out.points4, 0, sizeof(float) * 4 * static_cast<size_t>(n));
    if (out.cands) memset(out.cands, 0, sizeof(double) * f.ids * f.words);
    if (out.counts) for (int j = 0; j < f.ids; ++j) out.counts[j] = -1;
    if (out.n_models) *out.n_models = 0;
    if (out.E_ref) memset(out.E_ref, 0, sizeof(double) * 9);
}

// Driver of every host-pointer form: n correspondences a1 (dim1 floats each), a2 (dim2 floats each).  RANSAC over p's
// samples (or CANDIDATES), then (SECOND) the second step on its winner and mask; SECOND alone: on the caller's model
// (model_in, tail_in) and mask_in (pose recovery: mask_in may be null).  The outputs are reset before the first check,
// except that a refit or refinement alone first needs its model pointers (out.model may alias model_in).
int run_host(pm_ctx* ctx, const Family& f, int steps, const float* a1, const float* a2, int n, const pm_camera* K,
             const pm_ransac_params* p, const uint8_t* mask_in, const double* model_in, const double* tail_in,
             const HostOut& out)
{
    const bool ransac = steps & (RANSAC | CANDIDATES), second = steps & SECOND, cands = steps & CANDIDATES;
    const bool refit_alone = !ransac && !f.pose();
    const size_t model_bytes = sizeof(double) * static_cast<size_t>(f.words), mask_bytes = n > 0 ? n : 0;
    double in[13] = {};
    if (refit_alone)
        PM_REQUIRE(model_in && out.model && (f.words <= 9 || (tail_in && out.tail)), PM_E_INVALID, f.null_model);
    if (!ransac && model_in) {
        memcpy(in, model_in, sizeof(double) * (f.words < 9 ? f.words : 9));
        if (tail_in) memcpy(in + 9, tail_in, sizeof(double) * (f.words - 9));
    }
    reset_outputs(f, ransac, n, in, out);
    float thr = 1.0f;
    int rc = check_args(f, steps, p, K, model_in, &thr);
    if (rc != PM_OK) return rc;
    if (cands) PM_REQUIRE(out.cands && out.counts, PM_E_INVALID, f.null_cands);
    PM_REQUIRE(n >= 0 && (n == 0 || (a1 && a2 && (!refit_alone || mask_in))), PM_E_INVALID,
               refit_alone ? "bad point or mask arrays" : "bad point arrays");
    if (n < f.min_pts) {
        pm::set_error("need at least %d correspondences, got %d", f.min_pts, n);
        return PM_E_TOO_FEW;
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));

    // Arena: the two point arrays, the mask, points4, the results block, then what RANSAC carves (one slot set more per
    // candidate scored alone) and 1 KiB of slack on top of scratch_bytes()'s own: the most any family needs.
    const size_t b1 = sizeof(float) * f.dim1 * static_cast<size_t>(n), b2 = sizeof(float) * f.dim2 * static_cast<size_t>(n);
    const size_t pts = out.points4 ? sizeof(float) * 4 * static_cast<size_t>(n) : 0;
    const size_t res_bytes = results_bytes(f);
    rc = pm::arena_reserve(ctx, pm::align_up(b1, 256) + pm::align_up(b2, 256) + pm::align_up(mask_bytes, 256) +
                                    pm::align_up(pts, 256) + pm::align_up(res_bytes, 256) +
                                    (ransac ? scratch_bytes(ctx, f, n, p, thr) : 0) + (cands ? f.ids * 1024 : 0) + 1024);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    float* d1 = static_cast<float*>(pm::arena_take(ctx, b1));
    float* d2 = static_cast<float*>(pm::arena_take(ctx, b2));
    uint8_t* dmask = static_cast<uint8_t*>(pm::arena_take(ctx, mask_bytes));
    float* dpts = pts ? static_cast<float*>(pm::arena_take(ctx, pts)) : nullptr;
    void* dblock = pm::arena_take(ctx, res_bytes);
    PM_REQUIRE(d1 && d2 && dmask && dblock && (dpts || !pts), PM_E_NOMEM, "scratch arena too small");
    rc = pm::pinned_reserve(ctx, res_bytes + mask_bytes + pts);
    if (rc != PM_OK) return rc;
    const Results dres = results_at(f, dblock), hres = results_at(f, ctx->pinned);
    uint8_t* hmask = static_cast<uint8_t*>(ctx->pinned) + res_bytes;
    uint8_t* hpts = hmask + n;

    PM_HIP_CHECK(hipMemcpyAsync(d1, a1, b1, hipMemcpyHostToDevice, ctx->stream));
    PM_HIP_CHECK(hipMemcpyAsync(d2, a2, b2, hipMemcpyHostToDevice, ctx->stream));
    if (!ransac) {
        memcpy(hres.model, in, model_bytes);
        // H, A and X send the mask before the model, E and P after it
        const bool mask_first = f.id == H || f.id == A || f.id == F || f.id == X;
        if (mask_first) PM_HIP_CHECK(hipMemcpyAsync(dmask, mask_in, mask_bytes, hipMemcpyHostToDevice, ctx->stream));
        PM_HIP_CHECK(hipMemcpyAsync(dres.model, hres.model, model_bytes, hipMemcpyHostToDevice, ctx->stream));
        if (!mask_first && mask_in)
            PM_HIP_CHECK(hipMemcpyAsync(dmask, mask_in, mask_bytes, hipMemcpyHostToDevice, ctx->stream));
    }
    const pm_points_view v{d1, d2, nullptr, 1, n, 0, 1, 0};      // one part, no device-side count
    if (cands)
        rc = enqueue_candidates(ctx, f, v, K, p, thr, dres, dmask);
    else if (ransac)
        rc = enqueue_ransac(ctx, f, v, K, p, thr, dres.key, dres.model, dmask, n, dres.count);
    if (rc != PM_OK) return rc;
    if (second && f.pose()) {
        rc = recover_pose_enqueue(ctx, v, *K, dres.model, (ransac || mask_in) ? dmask : nullptr, f.dist, dres.pose,
                                  dres.pose + 9, dmask, n, dres.n_good, dpts);
        if (rc == PM_OK && f.third)      // on the pose mask, in place
            rc = pose_refine_enqueue(ctx, v, *K, dmask, dres.pose, f.max_iters, dres.pose, dres.E_ref, dres.info3);
    } else if (second) {
        rc = enqueue_refine(ctx, f, v, K, dmask, dres.model, dres.model, dres.info, f.id == R ? dres.E_ref : nullptr);
    }
    if (rc != PM_OK) return rc;
    PM_HIP_CHECK(hipMemcpyAsync(hres.key, dres.key, res_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (!refit_alone) PM_HIP_CHECK(hipMemcpyAsync(hmask, dmask, mask_bytes, hipMemcpyDeviceToHost, ctx->stream));
    if (pts) PM_HIP_CHECK(hipMemcpyAsync(hpts, dpts, pts, hipMemcpyDeviceToHost, ctx->stream));
    PM_HIP_CHECK(hipStreamSynchronize(ctx->stream));

    if (cands) {
        int nm = 0;
        for (int j = 0; j < f.ids; ++j) {
            if (hres.cand[f.stride * j + f.flag] == 0.0) continue;
            memcpy(out.cands + f.words * j, hres.cand + f.stride * j, model_bytes);
            out.counts[j] = static_cast<int32_t>(hres.keys[j] >> 32);
            ++nm;
        }
        if (out.n_models) *out.n_models = nm;
        if (nm == 0) {
            pm::set_error("no valid candidate (degenerate sample)");
            return PM_E_NO_MODEL;
        }
        return PM_OK;
    }
    if (ransac) {
        if (out.best_key) *out.best_key = *hres.key;
        if (out.info)
            *out.info = second ? *(f.third ? hres.info3 : hres.info) : pm_h_refine_info{0.0, 0.0, 0, 0, *hres.key ? 1 : 2, 0};
        if (*hres.key == 0ull) {
            pm::set_error("no valid model (all %s degenerate)", f.unit);
            return PM_E_NO_MODEL;
        }
        put_model(f, out, hres.model);
        if (out.n_inliers) *out.n_inliers = *hres.count;
    } else if (refit_alone) {
        put_model(f, out, hres.model);
        if (out.info) *out.info = *hres.info;
        if (out.E_ref) memcpy(out.E_ref, hres.E_ref, sizeof(double) * 9);
        if (hres.info->status == 2) {
            pm::set_error("the input %s is zero (no model)", f.name);
            return PM_E_NO_MODEL;
        }
    }
    if (second && f.pose()) {
        const double* t = hres.pose + 9;
        if (t[0] == 0.0 && t[1] == 0.0 && t[2] == 0.0) {
            pm::set_error("E does not decompose (rank < 2 or not finite)");
            return PM_E_NO_MODEL;
        }
        if (out.R) memcpy(out.R, hres.pose, sizeof(double) * 9);
        if (out.t) memcpy(out.t, t, sizeof(double) * 3);
        if (f.third && out.model) memcpy(out.model, hres.E_ref, sizeof(double) * 9);      // the E of the refined pose
        if (out.n_good) *out.n_good = *hres.n_good;
        if (out.points4) memcpy(out.points4, hpts, pts);
    }
    if (out.mask) memcpy(out.mask, hmask, mask_bytes);
    return PM_OK;
}

// The model, mask and count of hypothesis id `hyp` alone (H, A, X): RANSAC over [hyp, hyp + 1)
int run_host_hyp(pm_ctx* ctx, const Family& f, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                 int64_t hyp, double* model, uint8_t* mask, int* n_inliers)
{
    if (model) memset(model, 0, sizeof(double) * static_cast<size_t>(f.words));
    if (n_inliers) *n_inliers = 0;
    PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL, PM_E_INVALID, "hypothesis id must satisfy 0 <= hyp < 2^32");
    PM_REQUIRE(p != nullptr, PM_E_INVALID, "params is null");
    pm_ransac_params q = *p;
    q.hyp_begin = hyp;
    q.hyp_end = hyp + 1;
    return run_host(ctx, f, RANSAC, xy1, xy2, n, nullptr, &q, nullptr, nullptr, nullptr,
                    HostOut{model, mask, n_inliers, nullptr, nullptr, model && f.words > 9 ? model + 9 : nullptr});
}

// Every candidate of sample id `hyp` with its count (E, P): CANDIDATES over [hyp, hyp + 1).  E refuses a bad hyp itself,
// before it looks at p; P leaves it to the range check.
int run_host_candidates(pm_ctx* ctx, const Family& f, const float* a1, const float* a2, int n, const pm_camera* K,
                        const pm_ransac_params* p, int64_t hyp, double* models, int32_t* counts, int* n_models)
{
    HostOut o{};
    o.cands = models; o.counts = counts; o.n_models = n_models;
    if (f.id == E) {
        const double zero[12] = {};
        reset_outputs(f, true, n, zero, o);
        PM_REQUIRE(hyp >= 0 && hyp < 0x100000000LL / 10, PM_E_INVALID,
                   "sample id must satisfy 0 <= hyp and 10 * hyp + 10 <= 2^32");
    }
    pm_ransac_params q{};
    if (p) {
        q = *p;
        q.hyp_begin = hyp;
        q.hyp_end = hyp + 1;
    }
    return run_host(ctx, f, CANDIDATES, a1, a2, n, K, p ? &q : nullptr, nullptr, nullptr, nullptr, o);
}

// The view of a device form: a pm_points_view (H, A, E), a pm_pnp_view (P) or a pm_xyz_view (X)
struct DevView {
    const pm_points_view* xy;
    const pm_pnp_view* pnp;
    const pm_xyz_view* xyz;
};

// The device forms' checks after the family's: the view (*v: as the launches take it), ctx; then the device and
// (RANSAC, p checked) the arena for what RANSAC carves.
int dev_prologue(pm_ctx* ctx, const Family& f, const DevView& view, const pm_ransac_params* p, float thr, pm_points_view* v)
{
    if (f.id == P) {
        PM_REQUIRE(view.pnp != nullptr && view.pnp->xyz && view.pnp->uv && view.pnp->cap >= 1, PM_E_INVALID,
                   "need a view with points and cap >= 1");
        *v = pm_points_view{view.pnp->xyz, view.pnp->uv, view.pnp->count, 1, view.pnp->cap, 0, 1, 0};
    } else if (f.id == X) {
        PM_REQUIRE(view.xyz != nullptr && view.xyz->xyz1 && view.xyz->xyz2 && view.xyz->cap >= 1, PM_E_INVALID,
                   "need a view with points and cap >= 1");
        *v = pm_points_view{view.xyz->xyz1, view.xyz->xyz2, view.xyz->count, 1, view.xyz->cap, 0, 1, 0};
    } else {
        const int rc = check_view(view.xy);
        if (rc != PM_OK) return rc;
        *v = *view.xy;
    }
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    if (!p) return PM_OK;
    // both before anything is enqueued: on a capturing stream either may refuse (E, P and X launch their solver first)
    int rc = pm::arena_reserve(ctx, scratch_bytes(ctx, f, static_cast<long long>(v->parts) * v->cap, p, thr));
    if (rc == PM_OK) rc = pm::sync_words_reserve(ctx);
    if (rc != PM_OK) return rc;
    pm::arena_reset(ctx);
    return PM_OK;
}

int run_dev(pm_ctx* ctx, const Family& f, const DevView& view, const pm_camera* K, const pm_ransac_params* p,
            uint64_t* d_best_key, double* d_model, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers)
{
    PM_REQUIRE(d_best_key && d_model && d_mask && d_n_inliers, PM_E_INVALID, "null argument");
    PM_REQUIRE(mask_len >= 0, PM_E_INVALID, "mask_len must be >= 0");
    float thr = 1.0f;
    int rc = check_args(f, RANSAC, p, K, nullptr, &thr);
    if (rc != PM_OK) return rc;
    pm_points_view v{};
    rc = dev_prologue(ctx, f, view, p, thr, &v);
    if (rc != PM_OK) return rc;
    return enqueue_ransac(ctx, f, v, K, p, thr, reinterpret_cast<unsigned long long*>(d_best_key), d_model, d_mask,
                          mask_len, d_n_inliers);
}

// The second step alone on device arrays; `required`: the entry point's non-optional pointers are all there
int second_dev(pm_ctx* ctx, const Family& f, const DevView& view, const pm_camera* K, bool required, const double* d_in,
               pm_points_view* v)
{
    PM_REQUIRE(required, PM_E_INVALID, "null argument");
    float thr = 1.0f;
    const int rc = check_args(f, SECOND, nullptr, K, d_in, &thr);
    if (rc != PM_OK) return rc;
    return dev_prologue(ctx, f, view, nullptr, thr, v);
}

int refine_dev(pm_ctx* ctx, const Family& f, const DevView& view, const pm_camera* K, const uint8_t* d_mask,
               const double* d_in, double* d_out, pm_h_refine_info* d_info)
{
    pm_points_view v{};
    const int rc = second_dev(ctx, f, view, K, d_mask && d_in && d_out, d_in, &v);
    if (rc != PM_OK) return rc;
    return enqueue_refine(ctx, f, v, K, d_mask, d_in, d_out, d_info);
}

}  // namespace
}  // namespace pm_ransac

using namespace pm_ransac;

// ---- robust homography
extern "C" int pm_ransac_homography(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_ransac_params* p,
                                    double H[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return run_host(ctx, homography(0), RANSAC, xy1, xy2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{H, mask, n_inliers, best_key, nullptr});
}

extern "C" int pm_ransac_homography_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                             const pm_ransac_params* p, int64_t hyp, double H[9], uint8_t* mask,
                                             int* n_inliers)
{
    return run_host_hyp(ctx, homography(0), xy1, xy2, n, p, hyp, H, mask, n_inliers);
}

extern "C" int pm_ransac_homography_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_ransac_params* p,
                                            uint64_t* d_best_key, double* d_H, uint8_t* d_mask, int mask_len,
                                            int32_t* d_n_inliers)
{
    return run_dev(ctx, homography(0), DevView{view, nullptr, nullptr}, nullptr, p, d_best_key, d_H, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_homography_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                                    const double H_in[9], int max_iters, double H_out[9], pm_h_refine_info* info)
{
    return run_host(ctx, homography(max_iters), SECOND, xy1, xy2, n, nullptr, nullptr, mask, H_in, nullptr,
                    HostOut{H_out, nullptr, nullptr, nullptr, info});
}

extern "C" int pm_homography_refine_dev(pm_ctx* ctx, const pm_points_view* view, const uint8_t* d_mask,
                                        const double* d_H_in, int max_iters, double* d_H_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, homography(max_iters), DevView{view, nullptr, nullptr}, nullptr, d_mask, d_H_in, d_H_out, d_info);
}

extern "C" int pm_ransac_homography_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                            const pm_ransac_params* p, int max_iters, double H[9], uint8_t* mask,
                                            int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, homography(max_iters), RANSAC | SECOND, xy1, xy2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{H, mask, n_inliers, best_key, info});
}

// ---- robust affine / similarity
extern "C" int pm_ransac_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                const pm_ransac_params* p, double A[6], uint8_t* mask, int* n_inliers,
                                uint64_t* best_key)
{
    return run_host(ctx, affine(model), RANSAC, xy1, xy2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{A, mask, n_inliers, best_key, nullptr});
}

extern "C" int pm_ransac_affine_from_hyp(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                         const pm_ransac_params* p, int64_t hyp, double A[6], uint8_t* mask,
                                         int* n_inliers)
{
    return run_host_hyp(ctx, affine(model), xy1, xy2, n, p, hyp, A, mask, n_inliers);
}

extern "C" int pm_ransac_affine_run_dev(pm_ctx* ctx, int model, const pm_points_view* view, const pm_ransac_params* p,
                                        uint64_t* d_best_key, double* d_A, uint8_t* d_mask, int mask_len,
                                        int32_t* d_n_inliers)
{
    return run_dev(ctx, affine(model), DevView{view, nullptr, nullptr}, nullptr, p, d_best_key, d_A, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_affine_refine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                                const double A_in[6], double A_out[6], pm_h_refine_info* info)
{
    return run_host(ctx, affine(model), SECOND, xy1, xy2, n, nullptr, nullptr, mask, A_in, nullptr,
                    HostOut{A_out, nullptr, nullptr, nullptr, info});
}

extern "C" int pm_affine_refine_dev(pm_ctx* ctx, int model, const pm_points_view* view, const uint8_t* d_mask,
                                    const double* d_A_in, double* d_A_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, affine(model), DevView{view, nullptr, nullptr}, nullptr, d_mask, d_A_in, d_A_out, d_info);
}

extern "C" int pm_estimate_affine(pm_ctx* ctx, int model, const float* xy1, const float* xy2, int n,
                                  const pm_ransac_params* p, int refine, double A[6], uint8_t* mask, int* n_inliers,
                                  uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, affine(model), refine ? RANSAC | SECOND : RANSAC, xy1, xy2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{A, mask, n_inliers, best_key, info});
}

// ---- calibrated relative pose
extern "C" int pm_ransac_essential(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                   const pm_ransac_params* p, double E[9], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    return run_host(ctx, essential(0.0), RANSAC, xy1, xy2, n, K, p, nullptr, nullptr, nullptr,
                    HostOut{E, mask, n_inliers, best_key, nullptr});
}

extern "C" int pm_ransac_essential_from_hyp(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                            const pm_ransac_params* p, int64_t hyp, double E[90], int32_t counts[10],
                                            int* n_models)
{
    return run_host_candidates(ctx, essential(0.0), xy1, xy2, n, K, p, hyp, E, counts, n_models);
}

extern "C" int pm_ransac_essential_run_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K,
                                           const pm_ransac_params* p, uint64_t* d_best_key, double* d_E, uint8_t* d_mask,
                                           int mask_len, int32_t* d_n_inliers)
{
    return run_dev(ctx, essential(0.0), DevView{view, nullptr, nullptr}, K, p, d_best_key, d_E, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_recover_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K, const double E[9],
                               const uint8_t* mask_in, double dist, double R[9], double t[3], uint8_t* mask_out, int* n_good,
                               float* points4)
{
    return run_host(ctx, essential(dist), SECOND, xy1, xy2, n, K, nullptr, mask_in, E, nullptr,
                    HostOut{nullptr, mask_out, nullptr, nullptr, nullptr, nullptr, R, t, n_good, points4});
}

extern "C" int pm_recover_pose_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const double* d_E,
                                   const uint8_t* d_mask_in, double dist, double* d_R, double* d_t, uint8_t* d_mask_out,
                                   int32_t* d_n_good, float* d_points4)
{
    pm_points_view v{};
    const int rc = second_dev(ctx, essential(dist), DevView{view, nullptr, nullptr}, K, d_E && d_R && d_t && d_mask_out && d_n_good,
                              d_E, &v);
    if (rc != PM_OK) return rc;
    return recover_pose_enqueue(ctx, v, *K, d_E, d_mask_in, dist, d_R, d_t, d_mask_out, v.parts * v.cap, d_n_good,
                                d_points4);
}

extern "C" int pm_estimate_pose(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                const pm_ransac_params* p, double dist, double E[9], double R[9], double t[3], uint8_t* mask,
                                int* n_inliers, int* n_good, uint64_t* best_key)
{
    return run_host(ctx, essential(dist), RANSAC | SECOND, xy1, xy2, n, K, p, nullptr, nullptr, nullptr,
                    HostOut{E, mask, n_inliers, best_key, nullptr, nullptr, R, t, n_good});
}

extern "C" int pm_estimate_pose_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K,
                                        const pm_ransac_params* p, double dist, int max_iters, double E[9], double R[9],
                                        double t[3], uint8_t* mask, int* n_inliers, int* n_good, uint64_t* best_key,
                                        pm_h_refine_info* info)
{
    return run_host(ctx, essential(dist, true, max_iters), RANSAC | SECOND, xy1, xy2, n, K, p, nullptr, nullptr, nullptr,
                    HostOut{E, mask, n_inliers, best_key, info, nullptr, R, t, n_good});
}

extern "C" int pm_pose_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const pm_camera* K, const uint8_t* mask,
                              const double R_in[9], const double t_in[3], int max_iters, double R_out[9], double t_out[3],
                              double E_out[9], pm_h_refine_info* info)
{
    HostOut o{R_out, nullptr, nullptr, nullptr, info, t_out};
    o.E_ref = E_out;
    return run_host(ctx, relpose(max_iters), SECOND, xy1, xy2, n, K, nullptr, mask, R_in, t_in, o);
}

extern "C" int pm_pose_refine_dev(pm_ctx* ctx, const pm_points_view* view, const pm_camera* K, const uint8_t* d_mask,
                                  const double* d_Rt_in, int max_iters, double* d_Rt_out, double* d_E_out,
                                  pm_h_refine_info* d_info)
{
    const Family f = relpose(max_iters);
    pm_points_view v{};
    const int rc = second_dev(ctx, f, DevView{view, nullptr, nullptr}, K, d_mask && d_Rt_in && d_Rt_out, d_Rt_in, &v);
    if (rc != PM_OK) return rc;
    return enqueue_refine(ctx, f, v, K, d_mask, d_Rt_in, d_Rt_out, d_info, d_E_out);
}

// ---- fundamental matrix: refinement (RANSAC-F itself: ransac.hip)
extern "C" int pm_fundamental_refine(pm_ctx* ctx, const float* xy1, const float* xy2, int n, const uint8_t* mask,
                                     const double F_in[9], int max_iters, double F_out[9], pm_h_refine_info* info)
{
    return run_host(ctx, fundamental(max_iters), SECOND, xy1, xy2, n, nullptr, nullptr, mask, F_in, nullptr,
                    HostOut{F_out, nullptr, nullptr, nullptr, info});
}

extern "C" int pm_fundamental_refine_dev(pm_ctx* ctx, const pm_points_view* view, const uint8_t* d_mask,
                                         const double* d_F_in, int max_iters, double* d_F_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, fundamental(max_iters), DevView{view, nullptr, nullptr}, nullptr, d_mask, d_F_in, d_F_out, d_info);
}

extern "C" int pm_ransac_fundamental_refined(pm_ctx* ctx, const float* xy1, const float* xy2, int n,
                                             const pm_ransac_params* p, int max_iters, double F[9], uint8_t* mask,
                                             int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, fundamental(max_iters), RANSAC | SECOND, xy1, xy2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{F, mask, n_inliers, best_key, info});
}

// ---- absolute pose
extern "C" int pm_ransac_pnp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                             const pm_ransac_params* p, double R[9], double t[3], uint8_t* mask, int* n_inliers,
                             uint64_t* best_key)
{
    return run_host(ctx, pnp(0), RANSAC, xyz, uv, n, K, p, nullptr, nullptr, nullptr,
                    HostOut{R, mask, n_inliers, best_key, nullptr, t});
}

extern "C" int pm_ransac_pnp_from_hyp(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                                      const pm_ransac_params* p, int64_t hyp, double Rt[48], int32_t counts[4], int* n_models)
{
    return run_host_candidates(ctx, pnp(0), xyz, uv, n, K, p, hyp, Rt, counts, n_models);
}

extern "C" int pm_ransac_pnp_run_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const pm_ransac_params* p,
                                     uint64_t* d_best_key, double* d_Rt, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers)
{
    return run_dev(ctx, pnp(0), DevView{nullptr, view, nullptr}, K, p, d_best_key, d_Rt, d_mask, mask_len, d_n_inliers);
}

extern "C" int pm_pnp_refine(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K, const uint8_t* mask,
                             const double R_in[9], const double t_in[3], int max_iters, double R_out[9], double t_out[3],
                             pm_h_refine_info* info)
{
    return run_host(ctx, pnp(max_iters), SECOND, xyz, uv, n, K, nullptr, mask, R_in, t_in,
                    HostOut{R_out, nullptr, nullptr, nullptr, info, t_out});
}

extern "C" int pm_pnp_refine_dev(pm_ctx* ctx, const pm_pnp_view* view, const pm_camera* K, const uint8_t* d_mask,
                                 const double* d_Rt_in, int max_iters, double* d_Rt_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, pnp(max_iters), DevView{nullptr, view, nullptr}, K, d_mask, d_Rt_in, d_Rt_out, d_info);
}

extern "C" int pm_solve_pnp_ransac(pm_ctx* ctx, const float* xyz, const float* uv, int n, const pm_camera* K,
                                   const pm_ransac_params* p, int max_iters, double R[9], double t[3], uint8_t* mask,
                                   int* n_inliers, uint64_t* best_key, pm_h_refine_info* info)
{
    return run_host(ctx, pnp(max_iters), RANSAC | SECOND, xyz, uv, n, K, p, nullptr, nullptr, nullptr,
                    HostOut{R, mask, n_inliers, best_key, info, t});
}

extern "C" int pm_gather_pnp_dev(pm_ctx* ctx, const pm_match* d_matches, const int32_t* d_count, int cap, const float* d_kp_xy,
                                 int n_kp, const float* d_obj_xyz, int n_obj, float* d_uv, float* d_xyz)
{
    PM_REQUIRE(d_matches && d_kp_xy && d_obj_xyz && d_uv && d_xyz, PM_E_INVALID, "null argument");
    PM_REQUIRE(cap >= 1 && n_kp >= 0 && n_obj >= 0, PM_E_INVALID, "need cap >= 1, n_kp >= 0, n_obj >= 0");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return gather_pnp_enqueue(ctx, d_matches, d_count, cap, d_kp_xy, n_kp, d_obj_xyz, n_obj, d_uv, d_xyz);
}

// ---- 3-D to 3-D alignment
namespace {
double* tail13(double* T) { return T ? T + 9 : nullptr; }
const double* tail13(const double* T) { return T ? T + 9 : nullptr; }
}  // namespace

extern "C" int pm_ransac_align3d(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n, const pm_ransac_params* p,
                                 double T[13], uint8_t* mask, int* n_inliers, uint64_t* best_key)
{
    const Family f = align3d(model);
    if (!T) {
        const double zero[13] = {};
        reset_outputs(f, true, n, zero, HostOut{nullptr, mask, n_inliers, best_key, nullptr});
        PM_REQUIRE(T != nullptr, PM_E_INVALID, "null T");
    }
    return run_host(ctx, f, RANSAC, xyz1, xyz2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{T, mask, n_inliers, best_key, nullptr, tail13(T)});
}

extern "C" int pm_ransac_align3d_from_hyp(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n,
                                          const pm_ransac_params* p, int64_t hyp, double T[13], uint8_t* mask, int* n_inliers)
{
    if (!T) {
        if (n_inliers) *n_inliers = 0;
        if (mask && n > 0) memset(mask, 0, static_cast<size_t>(n));
        PM_REQUIRE(T != nullptr, PM_E_INVALID, "null T");
    }
    return run_host_hyp(ctx, align3d(model), xyz1, xyz2, n, p, hyp, T, mask, n_inliers);
}

extern "C" int pm_ransac_align3d_run_dev(pm_ctx* ctx, int model, const pm_xyz_view* view, const pm_ransac_params* p,
                                         uint64_t* d_best_key, double* d_T, uint8_t* d_mask, int mask_len, int32_t* d_n_inliers)
{
    return run_dev(ctx, align3d(model), DevView{nullptr, nullptr, view}, nullptr, p, d_best_key, d_T, d_mask, mask_len,
                   d_n_inliers);
}

extern "C" int pm_align3d_refine(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n, const uint8_t* mask,
                                 const double T_in[13], double T_out[13], pm_h_refine_info* info)
{
    return run_host(ctx, align3d(model), SECOND, xyz1, xyz2, n, nullptr, nullptr, mask, T_in, tail13(T_in),
                    HostOut{T_out, nullptr, nullptr, nullptr, info, tail13(T_out)});
}

extern "C" int pm_align3d_refine_dev(pm_ctx* ctx, int model, const pm_xyz_view* view, const uint8_t* d_mask,
                                     const double* d_T_in, double* d_T_out, pm_h_refine_info* d_info)
{
    return refine_dev(ctx, align3d(model), DevView{nullptr, nullptr, view}, nullptr, d_mask, d_T_in, d_T_out, d_info);
}

extern "C" int pm_estimate_align3d(pm_ctx* ctx, int model, const float* xyz1, const float* xyz2, int n,
                                   const pm_ransac_params* p, int refine, double T[13], uint8_t* mask, int* n_inliers,
                                   uint64_t* best_key, pm_h_refine_info* info)
{
    const Family f = align3d(model);
    if (!T) {
        const double zero[13] = {};
        reset_outputs(f, true, n, zero, HostOut{nullptr, mask, n_inliers, best_key, info});
        PM_REQUIRE(T != nullptr, PM_E_INVALID, "null T");
    }
    return run_host(ctx, f, refine ? RANSAC | SECOND : RANSAC, xyz1, xyz2, n, nullptr, p, nullptr, nullptr, nullptr,
                    HostOut{T, mask, n_inliers, best_key, info, tail13(T)});
}

extern "C" int pm_gather_align3d_dev(pm_ctx* ctx, const pm_match* d_matches, const int32_t* d_count, int cap, const float* d_tab1,
                                     int n1, const float* d_tab2, int n2, float* d_xyz1, float* d_xyz2)
{
    PM_REQUIRE(d_matches && d_tab1 && d_tab2 && d_xyz1 && d_xyz2, PM_E_INVALID, "null argument");
    PM_REQUIRE(cap >= 1 && n1 >= 0 && n2 >= 0, PM_E_INVALID, "need cap >= 1, n1 >= 0, n2 >= 0");
    PM_REQUIRE(ctx != nullptr, PM_E_INVALID, "ctx is null");
    PM_HIP_CHECK(hipSetDevice(ctx->device));
    return gather_align3d_enqueue(ctx, d_matches, d_count, cap, d_tab1, n1, d_tab2, n2, d_xyz1, d_xyz2);
}
