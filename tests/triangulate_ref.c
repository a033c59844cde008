/* triangulate_ref.c — plain-C restatement of docs/SPEC.md S93-S96 (triangulation of map points from 2 .. 8 posed views:
 * observations, linear DLT, Levenberg-Marquardt over the point, gates).  Built by tests/cref.py with -ffp-contract=off; the
 * only fused multiply-adds are the fma() calls of libm, so the device kernel reproduces these bits.  Rows are indexed at
 * run time here; the kernel unrolls them. */
#include <math.h>
#include <stdint.h>

#define MAXV 8

enum { TR_OK = 0, TR_FEW_VIEWS = 1, TR_DEGENERATE = 2, TR_DEPTH = 3, TR_PARALLAX = 4, TR_REPROJ = 5 };
int tr_max_views(void) { return MAXV; }
int tr_use_initial(void) { return 1; }

/* S31 */
static float norm1(float p, double c, double f)
{
    const float v = (float)(((double)p - c) / f);
    return fabsf(v) <= 1048576.0f ? v : NAN;
}

/* S7 step 4 / S35: one rotation of columns p, q of G (rows x 4) and V (4 x 4) */
static void jacobi(double (*G)[4], int rows, double V[4][4], int p, int q)
{
    double al = G[0][p] * G[0][p], be = G[0][q] * G[0][q], ga = G[0][p] * G[0][q];
    for (int i = 1; i < rows; ++i) {
        al = fma(G[i][p], G[i][p], al);
        be = fma(G[i][q], G[i][q], be);
        ga = fma(G[i][p], G[i][q], ga);
    }
    if (!(ga * ga > 4.930380657631324e-32 * (al * be))) return;
    const double zeta = (be - al) / (2.0 * ga);
    const double t = (zeta >= 0.0 ? 1.0 : -1.0) / (fabs(zeta) + sqrt(fma(zeta, zeta, 1.0)));
    const double c = 1.0 / sqrt(fma(t, t, 1.0));
    const double s = c * t;
    for (int i = 0; i < rows; ++i) {
        const double gp = G[i][p], gq = G[i][q];
        G[i][p] = fma(c, gp, -(s * gq));
        G[i][q] = fma(s, gp, c * gq);
    }
    for (int i = 0; i < 4; ++i) {
        const double vp = V[i][p], vq = V[i][q];
        V[i][p] = fma(c, vp, -(s * vq));
        V[i][q] = fma(s, vp, c * vq);
    }
}

static double colnorm2(double (*G)[4], int rows, int p)
{
    double a = G[0][p] * G[0][p];
    for (int i = 1; i < rows; ++i) a = fma(G[i][p], G[i][p], a);
    return a;
}

/* S94 on `rows` rows */
static void null_vector(double (*A)[4], int rows, double Q[4])
{
    double V[4][4];
    for (int r = 0; r < 4; ++r)
        for (int c = 0; c < 4; ++c) V[r][c] = r == c ? 1.0 : 0.0;
    for (int s = 0; s < 8; ++s) {
        jacobi(A, rows, V, 0, 1); jacobi(A, rows, V, 0, 2); jacobi(A, rows, V, 0, 3);
        jacobi(A, rows, V, 1, 2); jacobi(A, rows, V, 1, 3); jacobi(A, rows, V, 2, 3);
    }
    int m = 0;
    double cm = colnorm2(A, rows, 0);
    for (int p = 1; p < 4; ++p) {
        const double c = colnorm2(A, rows, p);
        if (c < cm) { cm = c; m = p; }
    }
    for (int i = 0; i < 4; ++i) Q[i] = V[i][m];
}

/* the rows the linear stage would solve, for the numpy comparison: A is 2 * nv x 4 */
void tr_rows(const double* K, const float* const* uv, const double* const* Rt, int nv, int i, double* Aout);

typedef struct {
    double H[6], g[3], cost;
    int depth_ok;
} Pass;

/* S95: one pass at X */
static void lm_pass(const double* K, double P[MAXV][12], float pix[MAXV][2], const int* obs, int nv, const double X[3], Pass* o)
{
    for (int e = 0; e < 6; ++e) o->H[e] = 0.0;
    for (int e = 0; e < 3; ++e) o->g[e] = 0.0;
    o->cost = 0.0;
    o->depth_ok = 1;
    for (int v = 0; v < nv; ++v) {
        if (!obs[v]) continue;
        double xc[3];
        for (int r = 0; r < 3; ++r) xc[r] = ((P[v][3 * r] * X[0] + P[v][3 * r + 1] * X[1]) + P[v][3 * r + 2] * X[2]) + P[v][9 + r];
        if (!(xc[2] > 0.0 && xc[2] < INFINITY)) { o->depth_ok = 0; o->cost = INFINITY; return; }
        const double iz = 1.0 / xc[2];
        const double px = xc[0] * iz, py = xc[1] * iz;
        const double ru = (K[0] * px + K[2]) - (double)pix[v][0];
        const double rv = (K[1] * py + K[3]) - (double)pix[v][1];
        const double fa = K[0] * iz, fb = K[1] * iz;
        const double a = fa * px, b = fb * py;
        double ju[3], jv[3];
        for (int c = 0; c < 3; ++c) {
            ju[c] = fa * P[v][c] - a * P[v][6 + c];
            jv[c] = fb * P[v][3 + c] - b * P[v][6 + c];
        }
        int e = 0;
        for (int j = 0; j < 3; ++j)
            for (int q = j; q < 3; ++q, ++e) o->H[e] = o->H[e] + fma(ju[j], ju[q], jv[j] * jv[q]);
        for (int j = 0; j < 3; ++j) o->g[j] = o->g[j] + fma(ju[j], ru, jv[j] * rv);
        o->cost = o->cost + fma(ru, ru, rv * rv);
    }
}

/* S24's damped Cholesky at 3 parameters */
static int solve3(const double H[6], const double g[3], double lam, double d[3])
{
    static const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
    double L[3][3], y[3];
    for (int j = 0; j < 3; ++j) {
        const double ajj = H[at[j][j]];
        double dd = ajj + lam * ajj;
        for (int q = 0; q < j; ++q) dd = fma(-L[j][q], L[j][q], dd);
        if (!(dd > 0.0) || !(dd < INFINITY)) return 0;
        L[j][j] = sqrt(dd);
        for (int i = j + 1; i < 3; ++i) {
            double v = H[at[j][i]];
            for (int q = 0; q < j; ++q) v = fma(-L[i][q], L[j][q], v);
            L[i][j] = v / L[j][j];
        }
    }
    for (int i = 0; i < 3; ++i) {
        double v = -g[i];
        for (int q = 0; q < i; ++q) v = fma(-L[i][q], y[q], v);
        y[i] = v / L[i][i];
    }
    for (int i = 2; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 3; ++q) v = fma(-L[q][i], d[q], v);
        d[i] = v / L[i][i];
    }
    return 1;
}

static void load_pose(const double* Rt, double P[12])
{
    for (int j = 0; j < 12; ++j) P[j] = Rt ? Rt[j] : ((j < 9 && j % 4 == 0) ? 1.0 : 0.0);
}

static void view_rows(const double* Rt, const double P[12], int o, double x, double y, double r0[4], double r1[4])
{
    for (int c = 0; c < 4; ++c) {
        const double p0 = c < 3 ? P[c] : P[9], p1 = c < 3 ? P[3 + c] : P[10], p2 = c < 3 ? P[6 + c] : P[11];
        const double a0 = Rt ? x * p2 - p0 : (c == 0 ? -1.0 : (c == 2 ? x : 0.0));
        const double a1 = Rt ? y * p2 - p1 : (c == 1 ? -1.0 : (c == 2 ? y : 0.0));
        r0[c] = o ? a0 : 0.0;
        r1[c] = o ? a1 : 0.0;
    }
}

void tr_rows(const double* K, const float* const* uv, const double* const* Rt, int nv, int i, double* Aout)
{
    for (int v = 0; v < nv; ++v) {
        double P[12];
        load_pose(Rt[v], P);
        const float x = norm1(uv[v][2 * i], K[2], K[0]), y = norm1(uv[v][2 * i + 1], K[3], K[1]);
        view_rows(Rt[v], P, x == x && y == y, (double)x, (double)y, Aout + 8 * v, Aout + 8 * v + 4);
    }
}

/* The whole call over n points.  K = (fx, fy, cx, cy); prm = (max_reproj_px, max_cos_parallax, max_depth).  xyz is read
 * under flag 1.  points4, err2 may be NULL.  Extras for the CPU tests (may be NULL): cost_lin / cost_fin, the S95 cost at
 * the start and at the final point (NaN where refinement never looked), iters, the LM passes at trial points, xyz64, the
 * final point before the f32 rounding.  Returns n_good. */
int tr_run(const double* K, const float* const* uv, const double* const* Rt, int nv, int n, const double* prm, int max_iters,
           int flags, float* xyz, uint8_t* status, float* points4, float* err2, double* cost_lin, double* cost_fin,
           int32_t* iters, double* xyz64)
{
    const double thr2 = prm[0] * prm[0], max_cos = prm[1], max_depth = prm[2];
    double P[MAXV][12], C[MAXV][3];
    for (int v = 0; v < nv; ++v) {
        load_pose(Rt[v], P[v]);
        for (int c = 0; c < 3; ++c) C[v][c] = -((P[v][c] * P[v][9] + P[v][3 + c] * P[v][10]) + P[v][6 + c] * P[v][11]);
    }
    int good = 0;
    for (int i = 0; i < n; ++i) {
        float pix[MAXV][2];
        int obs[MAXV], seen = 0;
        double A[2 * MAXV][4];
        for (int v = 0; v < nv; ++v) {
            pix[v][0] = uv[v][2 * i];
            pix[v][1] = uv[v][2 * i + 1];
            const float x = norm1(pix[v][0], K[2], K[0]), y = norm1(pix[v][1], K[3], K[1]);
            obs[v] = x == x && y == y;
            seen += obs[v];
            view_rows(Rt[v], P[v], obs[v], (double)x, (double)y, A[2 * v], A[2 * v + 1]);
        }
        int st = TR_OK;
        double X[3];
        if (flags & 1) {
            for (int c = 0; c < 3; ++c) X[c] = (double)xyz[3 * i + c];
        } else {
            double Q[4];
            null_vector(A, 2 * nv, Q);
            if (points4)
                for (int c = 0; c < 4; ++c) points4[4 * i + c] = (float)Q[c];
            for (int c = 0; c < 3; ++c) X[c] = Q[c] / Q[3];
            if (Q[3] == 0.0) st = TR_DEGENERATE;
        }
        for (int c = 0; c < 3; ++c)
            if (!(fabs(X[c]) < INFINITY)) st = TR_DEGENERATE;
        if (seen < 2) st = TR_FEW_VIEWS;
        double err = 0.0, c_lin = NAN, c_fin = NAN;
        int it_used = 0;
        if (st == TR_OK) {
            Pass cur;
            lm_pass(K, P, pix, obs, nv, X, &cur);
            c_lin = cur.cost;
            if (cur.depth_ok && max_iters > 0) {
                double lam = 1e-3;
                for (int it = 0; it < max_iters; ++it) {
                    double d[3];
                    if (!solve3(cur.H, cur.g, lam, d)) break;
                    double dmax = 0.0, hmax = 1.0;
                    for (int c = 0; c < 3; ++c) {
                        if (!(fabs(d[c]) <= dmax)) dmax = fabs(d[c]);
                        if (!(fabs(X[c]) <= hmax)) hmax = fabs(X[c]);
                    }
                    if (!(dmax > 1e-15 * hmax)) break;
                    const double Xt[3] = {X[0] + d[0], X[1] + d[1], X[2] + d[2]};
                    Pass tr;
                    lm_pass(K, P, pix, obs, nv, Xt, &tr);
                    ++it_used;
                    if (tr.cost < cur.cost) {
                        cur = tr;
                        lam = lam / 10.0;
                        for (int c = 0; c < 3; ++c) X[c] = Xt[c];
                    } else {
                        lam = lam * 10.0;
                    }
                }
            }
            c_fin = cur.cost;
            /* S96 */
            int depth = 1, par = 1;
            double cmin = 1.0, r[MAXV][3], nn[MAXV];
            for (int v = 0; v < nv; ++v) {
                const double z = ((P[v][6] * X[0] + P[v][7] * X[1]) + P[v][8] * X[2]) + P[v][11];
                if (obs[v]) {
                    depth = depth && z > 0.0 && z < max_depth;
                    const double iz = 1.0 / z;
                    const double xu = ((P[v][0] * X[0] + P[v][1] * X[1]) + P[v][2] * X[2]) + P[v][9];
                    const double xv = ((P[v][3] * X[0] + P[v][4] * X[1]) + P[v][5] * X[2]) + P[v][10];
                    const double ru = (K[0] * (xu * iz) + K[2]) - (double)pix[v][0];
                    const double rv = (K[1] * (xv * iz) + K[3]) - (double)pix[v][1];
                    const double e = fma(ru, ru, rv * rv);
                    if (!(e <= err)) err = e;
                }
                for (int c = 0; c < 3; ++c) r[v][c] = X[c] - C[v][c];
                nn[v] = fma(r[v][0], r[v][0], fma(r[v][1], r[v][1], r[v][2] * r[v][2]));
            }
            for (int p = 0; p < nv; ++p)
                for (int q = p + 1; q < nv; ++q) {
                    if (!(obs[p] && obs[q])) continue;
                    const double dot = fma(r[p][0], r[q][0], fma(r[p][1], r[q][1], r[p][2] * r[q][2]));
                    const double cs = dot / sqrt(nn[p] * nn[q]);
                    par = par && cs == cs;
                    if (cs < cmin) cmin = cs;
                }
            if (!depth) st = TR_DEPTH;
            else if (max_cos < 1.0 && !(par && cmin < max_cos)) st = TR_PARALLAX;
            else if (!(err <= thr2)) st = TR_REPROJ;
        }
        const int ok = st == TR_OK;
        for (int c = 0; c < 3; ++c) xyz[3 * i + c] = ok ? (float)X[c] : NAN;
        status[i] = (uint8_t)st;
        if (err2) err2[i] = ok ? (float)err : NAN;
        if (cost_lin) cost_lin[i] = c_lin;
        if (cost_fin) cost_fin[i] = c_fin;
        if (iters) iters[i] = it_used;
        if (xyz64)
            for (int c = 0; c < 3; ++c) xyz64[3 * i + c] = X[c];
        good += ok;
    }
    return good;
}
