/* align3d_ref.c — plain-C restatement of docs/SPEC.md S97-S101 (3-D to 3-D alignment x2 = s R x1 + t: 3-sample, triad
 * solve, distance test, RANSAC winner, Horn / Umeyama refit on the inliers, the point transform).  Built with
 * -ffp-contract=off: the only fused multiply-adds are the explicit fma() / fmaf() calls, so every value is the bits the
 * HIP kernels (align3d_core.hpp, align3d_solve.hip, ransac_align3d_fused.hip, align3d_refine.hip) produce.  Loaded by
 * align3d_ref.py.  A model is 13 doubles: R (9, row-major), t (3), s (1); model 0 = rigid, 1 = similarity. */
#include <math.h>
#include <stdint.h>
#include <string.h>

#define WORDS 13

static uint64_t mix64(uint64_t z)
{
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}

/* S97 */
void ar_sample(uint64_t seed, uint64_t h, int n, int32_t* idx)
{
    const uint64_t stream = mix64(seed ^ 0x3C6EF372FE94F82BULL) ^ mix64(h + 0xA54FF53A5F1D36F1ULL);
    int cnt = 0;
    for (uint64_t d = 0; d < 64 && cnt < 3; ++d) {
        const uint64_t r = mix64(stream + (d + 1) * 0x9E3779B97F4A7C15ULL);
        const int c = (int)(((r >> 32) * (uint64_t)(uint32_t)n) >> 32);
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
    for (int c = 0; cnt < 3; ++c) {
        int rep = 0;
        for (int s = 0; s < cnt; ++s) rep |= idx[s] == c;
        if (!rep) idx[cnt++] = c;
    }
}

static double dot3(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }

static void cross3(const double* a, const double* b, double* o)
{
    o[0] = a[1] * b[2] - a[2] * b[1];
    o[1] = a[2] * b[0] - a[0] * b[2];
    o[2] = a[0] * b[1] - a[1] * b[0];
}

/* S38 step 5: orthonormal triad (e1, e2, n) of p0, p1, p2; 0 if a length is zero or not finite */
static int triad(const double* p0, const double* p1, const double* p2, double T[3][3])
{
    double d1[3], d2[3], nn[3];
    for (int i = 0; i < 3; ++i) { d1[i] = p1[i] - p0[i]; d2[i] = p2[i] - p0[i]; }
    cross3(d1, d2, nn);
    const double l1 = dot3(d1, d1), ln = dot3(nn, nn);
    if (!(l1 > 0.0) || !(l1 < INFINITY) || !(ln > 0.0) || !(ln < INFINITY)) return 0;
    const double i1 = 1.0 / sqrt(l1), in = 1.0 / sqrt(ln);
    for (int i = 0; i < 3; ++i) { T[0][i] = d1[i] * i1; T[2][i] = nn[i] * in; }
    cross3(T[2], T[0], T[1]);
    return 1;
}

/* S98 on 3 rows a (3 x 3 f32, frame 1) and b (frame 2): out (13, zero when invalid); returns the valid flag */
int ar_solve(int model, const float* a, const float* b, double* out)
{
    memset(out, 0, sizeof(double) * WORDS);
    double A[3][3], B[3][3], T1[3][3], T2[3][3];
    for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) { A[i][c] = (double)a[3 * i + c]; B[i][c] = (double)b[3 * i + c]; }
    if (!triad(A[0], A[1], A[2], T1) || !triad(B[0], B[1], B[2], T2)) return 0;
    double T[WORDS], ma[3], mb[3];
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) T[3 * r + c] = (T2[0][r] * T1[0][c] + T2[1][r] * T1[1][c]) + T2[2][r] * T1[2][c];
    for (int c = 0; c < 3; ++c) {
        ma[c] = ((A[0][c] + A[1][c]) + A[2][c]) / 3.0;
        mb[c] = ((B[0][c] + B[1][c]) + B[2][c]) / 3.0;
    }
    double s = 1.0;
    if (model == 1) {
        double qa = 0.0, qb = 0.0;
        for (int i = 0; i < 3; ++i) {
            double da[3], db[3];
            for (int c = 0; c < 3; ++c) { da[c] = A[i][c] - ma[c]; db[c] = B[i][c] - mb[c]; }
            qa = qa + dot3(da, da);
            qb = qb + dot3(db, db);
        }
        s = sqrt(qb / qa);
        if (!(s > 0.0) || !(s < INFINITY)) return 0;
    }
    T[12] = s;
    for (int r = 0; r < 3; ++r) T[9 + r] = mb[r] - s * ((T[3 * r] * ma[0] + T[3 * r + 1] * ma[1]) + T[3 * r + 2] * ma[2]);
    for (int i = 0; i < WORDS; ++i)
        if (!(fabs(T[i]) < INFINITY)) return 0;
    memcpy(out, T, sizeof T);
    return 1;
}

/* S99: M32 = (float)(s R | t), row r at P[4r .. 4r + 3] */
void ar_model32(const double* T, float* P)
{
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) P[4 * r + c] = (float)(T[12] * T[3 * r + c]);
        P[4 * r + 3] = (float)T[9 + r];
    }
}

static int inlier(const float* P, const float* a, const float* b, float thr2)
{
    const float x = a[0], y = a[1], z = a[2];
    const float ra = fmaf(P[0], x, fmaf(P[1], y, fmaf(P[2], z, P[3]))) - b[0];
    const float rb = fmaf(P[4], x, fmaf(P[5], y, fmaf(P[6], z, P[7]))) - b[1];
    const float rc = fmaf(P[8], x, fmaf(P[9], y, fmaf(P[10], z, P[11]))) - b[2];
    const float d2 = fmaf(ra, ra, fmaf(rb, rb, rc * rc));
    return d2 <= thr2 && d2 < INFINITY;
}

/* S99 of the model T over n correspondences: mask (may be NULL), returns the count */
int ar_score(const double* T, const float* x1, const float* x2, int n, float thr2, uint8_t* mask)
{
    float P[12];
    ar_model32(T, P);
    int c = 0;
    for (int i = 0; i < n; ++i) {
        const int in = inlier(P, x1 + 3 * i, x2 + 3 * i, thr2);
        if (mask) mask[i] = (uint8_t)in;
        c += in;
    }
    return c;
}

/* S97 + S98 of sample h: out (13); returns the valid flag (n < 3: invalid) */
int ar_candidate(int model, const float* x1, const float* x2, int n, uint64_t seed, uint64_t h, double* out)
{
    memset(out, 0, sizeof(double) * WORDS);
    if (n < 3) return 0;
    int32_t idx[3];
    ar_sample(seed, h, n, idx);
    float a[9], b[9];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) { a[3 * i + k] = x1[3 * idx[i] + k]; b[3 * i + k] = x2[3 * idx[i] + k]; }
    return ar_solve(model, a, b, out);
}

/* S100: whole run over samples [hyp_begin, hyp_end): the key; T (13), mask (n), count */
uint64_t ar_run(int model, const float* x1, const float* x2, int n, uint64_t seed, int64_t hyp_begin, int64_t hyp_end,
                float thresh, double* T, uint8_t* mask, int32_t* count)
{
    const float thr2 = thresh * thresh;
    uint64_t best = 0;
    double cand[WORDS];
    memset(T, 0, sizeof(double) * WORDS);
    for (int64_t h = hyp_begin; h < hyp_end; ++h) {
        if (!ar_candidate(model, x1, x2, n, seed, (uint64_t)h, cand)) continue;
        const int c = ar_score(cand, x1, x2, n, thr2, 0);
        const uint64_t key = ((uint64_t)(uint32_t)c << 32) | (uint64_t)(0xFFFFFFFFu - (uint32_t)h);
        if (key > best) { best = key; memcpy(T, cand, sizeof cand); }
    }
    *count = 0;
    if (mask) memset(mask, 0, (size_t)n);
    if (best) *count = ar_score(T, x1, x2, n, thr2, mask);
    return best;
}

/* ---- S101: the refit on the inliers --------------------------------------------------------------------------------- */
#define HR_P 512
#define NK 11
#define SWEEPS 10
#define GAP_REL 1e-9

/* S23's tree over the P partials */
static void reduce(double (*part)[NK], int nk, double* out)
{
    for (int s = HR_P / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p)
            for (int k = 0; k < nk; ++k) part[p][k] = part[p][k] + part[p + s][k];
    for (int k = 0; k < nk; ++k) out[k] = part[0][k];
}

/* row i as doubles; 0 unless all six values are finite */
static int row(const float* x1, const float* x2, int i, double* a, double* b)
{
    int ok = 1;
    for (int c = 0; c < 3; ++c) {
        a[c] = (double)x1[3 * i + c];
        b[c] = (double)x2[3 * i + c];
        ok = ok && fabs(a[c]) < INFINITY && fabs(b[c]) < INFINITY;
    }
    return ok;
}

static void cost_model(const double* T, double* M)
{
    for (int i = 0; i < 9; ++i) M[i] = T[12] * T[i];
    for (int i = 0; i < 3; ++i) M[9 + i] = T[9 + i];
}

static double cost_term(const double* M, const double* a, const double* b)
{
    double e[3];
    for (int k = 0; k < 3; ++k) e[k] = (((M[3 * k] * a[0] + M[3 * k + 1] * a[1]) + M[3 * k + 2] * a[2]) + M[9 + k]) - b[k];
    return fma(e[0], e[0], fma(e[1], e[1], e[2] * e[2]));
}

static void jacobi_rot(double A[4][4], double V[4][4], int P, int Q)
{
    const double apq = A[P][Q];
    if (apq == 0.0 || !(fabs(apq) < INFINITY)) return;
    const double theta = (A[Q][Q] - A[P][P]) / (2.0 * apq);
    const double t = (theta < 0.0 ? -1.0 : 1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
    const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
    for (int k = 0; k < 4; ++k) {
        const double akp = A[k][P], akq = A[k][Q];
        A[k][P] = c * akp - s * akq;
        A[k][Q] = s * akp + c * akq;
    }
    for (int k = 0; k < 4; ++k) {
        const double apk = A[P][k], aqk = A[Q][k];
        A[P][k] = c * apk - s * aqk;
        A[Q][k] = s * apk + c * aqk;
    }
    for (int k = 0; k < 4; ++k) {
        const double vkp = V[k][P], vkq = V[k][Q];
        V[k][P] = c * vkp - s * vkq;
        V[k][Q] = s * vkp + c * vkq;
    }
}

/* S101 steps 3-6 on the moments S[3r + c] = sum b_r a_c, qa = sum |a_c|^2 and the centroids; eig (may be NULL): the four
 * Jacobi eigenvalues.  Returns 0 when the rotation is not determined. */
int ar_horn(int model, const double* S, double qa, const double* ca, const double* cb, double* T, double* eig)
{
    const double Sxx = S[0], Sxy = S[3], Sxz = S[6], Syx = S[1], Syy = S[4], Syz = S[7], Szx = S[2], Szy = S[5], Szz = S[8];
    double A[4][4], V[4][4];
    A[0][0] = (Sxx + Syy) + Szz; A[0][1] = Syz - Szy; A[0][2] = Szx - Sxz; A[0][3] = Sxy - Syx;
    A[1][1] = (Sxx - Syy) - Szz; A[1][2] = Sxy + Syx; A[1][3] = Szx + Sxz;
    A[2][2] = (Syy - Sxx) - Szz; A[2][3] = Syz + Szy;
    A[3][3] = (Szz - Sxx) - Syy;
    for (int i = 0; i < 4; ++i)
        for (int j = 0; j < 4; ++j) {
            if (j < i) A[i][j] = A[j][i];
            V[i][j] = i == j ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < SWEEPS; ++sweep)
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) jacobi_rot(A, V, p, q);
    if (eig) for (int k = 0; k < 4; ++k) eig[k] = A[k][k];
    double l1 = A[0][0];
    int k1 = 0;
    for (int k = 1; k < 4; ++k)
        if (A[k][k] > l1) { l1 = A[k][k]; k1 = k; }
    double l2 = -INFINITY;
    for (int k = 0; k < 4; ++k)
        if (k != k1 && A[k][k] > l2) l2 = A[k][k];
    if (!(l1 > 0.0) || !(l1 < INFINITY) || !(l1 - l2 > GAP_REL * l1)) return 0;
    const double w = V[0][k1], x = V[1][k1], y = V[2][k1], z = V[3][k1];
    const double ww = w * w, xx = x * x, yy = y * y, zz = z * z;
    const double iq = 1.0 / (((ww + xx) + yy) + zz);
    T[0] = (((ww + xx) - yy) - zz) * iq; T[1] = (2.0 * (x * y - w * z)) * iq; T[2] = (2.0 * (x * z + w * y)) * iq;
    T[3] = (2.0 * (x * y + w * z)) * iq; T[4] = (((ww - xx) + yy) - zz) * iq; T[5] = (2.0 * (y * z - w * x)) * iq;
    T[6] = (2.0 * (x * z - w * y)) * iq; T[7] = (2.0 * (y * z + w * x)) * iq; T[8] = (((ww - xx) - yy) + zz) * iq;
    double s = 1.0;
    if (model == 1) {
        double num = 0.0;
        for (int i = 0; i < 9; ++i) num = num + T[i] * S[i];
        s = num / qa;
        if (!(s > 0.0) || !(s < INFINITY)) return 0;
    }
    T[12] = s;
    for (int r = 0; r < 3; ++r) T[9 + r] = cb[r] - s * ((T[3 * r] * ca[0] + T[3 * r + 1] * ca[1]) + T[3 * r + 2] * ca[2]);
    for (int i = 0; i < WORDS; ++i)
        if (!(fabs(T[i]) < INFINITY)) return 0;
    return 1;
}

/* S101: refit of T_in (13) on the correspondences with mask[i] != 0 and six finite values.  T_out (13, may alias T_in),
 * costs = (cost_in, cost_out), ints = (n_used, iters = 0, status) */
void ar_refine(int model, const float* x1, const float* x2, int n, const uint8_t* mask, const double* T_in, double* T_out,
               double* costs, int32_t* ints)
{
    static double part[HR_P][NK];
    double in[WORDS];
    memcpy(in, T_in, sizeof in);
    int zero = 1;
    for (int i = 0; i < WORDS; ++i) zero = zero && in[i] == 0.0;
    if (zero) {
        memcpy(T_out, in, sizeof in);
        costs[0] = costs[1] = 0.0;
        ints[0] = ints[1] = 0;
        ints[2] = 2;
        return;
    }
    double Min[12], red[NK], a[3], b[3];
    cost_model(in, Min);
    memset(part, 0, sizeof part);
    for (int i = 0; i < n; ++i) {
        if (!mask[i] || !row(x1, x2, i, a, b)) continue;
        double* acc = part[i % HR_P];
        acc[0] = acc[0] + 1.0;
        for (int c = 0; c < 3; ++c) { acc[1 + c] = acc[1 + c] + a[c]; acc[4 + c] = acc[4 + c] + b[c]; }
        acc[7] = acc[7] + cost_term(Min, a, b);
    }
    reduce(part, 8, red);
    const double nu = red[0], cost_in = red[7];
    double ca[3], cb[3];
    for (int c = 0; c < 3; ++c) { ca[c] = red[1 + c] / nu; cb[c] = red[4 + c] / nu; }
    double ref[WORDS] = {0};
    int ok_ref = 0;
    if (nu >= 3.0) {
        memset(part, 0, sizeof part);
        for (int i = 0; i < n; ++i) {
            if (!mask[i] || !row(x1, x2, i, a, b)) continue;
            double* acc = part[i % HR_P];
            double da[3], db[3];
            for (int c = 0; c < 3; ++c) { da[c] = a[c] - ca[c]; db[c] = b[c] - cb[c]; }
            for (int k = 0; k < 3; ++k)
                for (int c = 0; c < 3; ++c) acc[3 * k + c] = acc[3 * k + c] + db[k] * da[c];
            acc[9] = acc[9] + dot3(da, da);
            acc[10] = acc[10] + dot3(db, db);
        }
        reduce(part, 11, red);
        ok_ref = ar_horn(model, red, red[9], ca, cb, ref, 0);
    }
    double cost_out = cost_in;
    int accepted = 0;
    if (ok_ref) {
        double Mref[12];
        cost_model(ref, Mref);
        memset(part, 0, sizeof part);
        for (int i = 0; i < n; ++i) {
            if (!mask[i] || !row(x1, x2, i, a, b)) continue;
            part[i % HR_P][0] = part[i % HR_P][0] + cost_term(Mref, a, b);
        }
        reduce(part, 1, red);
        if (red[0] <= cost_in) { cost_out = red[0]; accepted = 1; }
    }
    memcpy(T_out, accepted ? ref : in, sizeof in);
    costs[0] = cost_in;
    costs[1] = cost_out;
    ints[0] = (int32_t)nu;
    ints[1] = 0;
    ints[2] = accepted ? 0 : 1;
}

/* S101 (points): out = (float)(s R x + t), fp64, one rounding; a non-finite input or result gives three quiet NaNs.
 * out may alias xyz. */
void ar_transform(const double* T, const float* xyz, int n, float* out)
{
    const double s = T[12];
    for (int i = 0; i < n; ++i) {
        const double x = (double)xyz[3 * i], y = (double)xyz[3 * i + 1], z = (double)xyz[3 * i + 2];
        double o[3];
        int fin = 1;
        for (int r = 0; r < 3; ++r) {
            o[r] = (((s * T[3 * r]) * x + (s * T[3 * r + 1]) * y) + (s * T[3 * r + 2]) * z) + T[9 + r];
            fin = fin && fabs(o[r]) < INFINITY;
        }
        for (int r = 0; r < 3; ++r) out[3 * i + r] = fin ? (float)o[r] : NAN;
    }
}
