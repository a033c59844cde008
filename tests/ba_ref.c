/* ba_ref.c — plain-C restatement of docs/SPEC.md S113-S117 (local bundle adjustment: the used set, the linearisation, the
 * Schur-complement Levenberg-Marquardt step over free poses and points, the result).  Built by tests/cref.py with
 * -ffp-contract=off; the only fused multiply-adds are the fma() calls of libm, so the device kernel reproduces these bits.
 * Sums over points keep S23's 512 partials and stride-halving tree; everything else is indexed at run time here. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define MAXV 8
#define NP 512
#define MAXM 42

int ba_max_views(void) { return MAXV; }

/* S31 */
static float norm1(float p, double c, double f)
{
    const float v = (float)(((double)p - c) / f);
    return fabsf(v) <= 1048576.0f ? v : NAN;
}

/* S23's tree over the 512 partials */
static double tree(double* part)
{
    for (int s = NP / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p) part[p] = part[p] + part[p + s];
    return part[0];
}

/* S114: the linearisation of one state */
typedef struct {
    double *Vp, *gp, *c, *W;          /* per point: 6, 3, 1 and F x 18 */
    double U[MAXV][21], gc[MAXV][6], cost;
} Lin;

typedef struct {
    double e, ru, rv, ju[6], jv[6], cu[3], cv[3];
    int depth_ok;
} Obs;

/* S114: one observation of the point X under the pose P */
static void observe(const double* K, const double* P, const double* X, const float* pix, Obs* o)
{
    double Y[3], xc[3];
    for (int r = 0; r < 3; ++r) {
        Y[r] = (P[3 * r] * X[0] + P[3 * r + 1] * X[1]) + P[3 * r + 2] * X[2];
        xc[r] = Y[r] + P[9 + r];
    }
    o->depth_ok = xc[2] > 0.0 && xc[2] < INFINITY;
    const double iz = 1.0 / xc[2];
    const double px = xc[0] * iz, py = xc[1] * iz;
    o->ru = (K[0] * px + K[2]) - (double)pix[0];
    o->rv = (K[1] * py + K[3]) - (double)pix[1];
    o->e = fma(o->ru, o->ru, o->rv * o->rv);
    const double fa = K[0] * iz, fb = K[1] * iz;
    const double a = fa * px, b = fb * py;
    o->ju[0] = -(a * Y[1]); o->ju[1] = fa * Y[2] + a * Y[0]; o->ju[2] = -(fa * Y[1]); o->ju[3] = fa; o->ju[4] = 0.0; o->ju[5] = -a;
    o->jv[0] = -(fb * Y[2]) - b * Y[1]; o->jv[1] = b * Y[0]; o->jv[2] = fb * Y[0]; o->jv[3] = 0.0; o->jv[4] = fb; o->jv[5] = -b;
    for (int c = 0; c < 3; ++c) {
        o->cu[c] = fa * P[c] - a * P[6 + c];
        o->cv[c] = fb * P[3 + c] - b * P[6 + c];
    }
}

static void linearise(const double* K, const float* const* uv, double P[MAXV][12], const double* X, const uint8_t* used, int n, int nv,
                      const int* fidx, int F, Lin* o)
{
    static double part[27][NP];
    int bad = 0;
    for (int i = 0; i < n; ++i) {
        if (!used[i]) continue;
        for (int e = 0; e < 6; ++e) o->Vp[6 * i + e] = 0.0;
        for (int e = 0; e < 3; ++e) o->gp[3 * i + e] = 0.0;
        o->c[i] = 0.0;
    }
    for (int v = 0; v < nv; ++v) {
        const int a = fidx[v];
        memset(part, 0, sizeof part);
        for (int i = 0; i < n; ++i) {
            if (!((used[i] >> v) & 1)) continue;
            Obs ob;
            observe(K, P[v], X + 3 * i, uv[v] + 2 * i, &ob);
            if (!ob.depth_ok) bad = 1;
            int e = 0;
            for (int j = 0; j < 3; ++j)
                for (int q = j; q < 3; ++q, ++e) o->Vp[6 * i + e] = o->Vp[6 * i + e] + fma(ob.cu[j], ob.cu[q], ob.cv[j] * ob.cv[q]);
            for (int j = 0; j < 3; ++j) o->gp[3 * i + j] = o->gp[3 * i + j] + fma(ob.cu[j], ob.ru, ob.cv[j] * ob.rv);
            o->c[i] = o->c[i] + ob.e;
            if (a < 0) continue;
            double* W = o->W + ((size_t)i * F + a) * 18;
            for (int j = 0; j < 6; ++j)
                for (int k = 0; k < 3; ++k) W[3 * j + k] = fma(ob.ju[j], ob.cu[k], ob.jv[j] * ob.cv[k]);
            e = 0;
            for (int j = 0; j < 6; ++j)
                for (int q = j; q < 6; ++q, ++e) part[e][i % NP] = part[e][i % NP] + fma(ob.ju[j], ob.ju[q], ob.jv[j] * ob.jv[q]);
            for (int j = 0; j < 6; ++j) part[21 + j][i % NP] = part[21 + j][i % NP] + fma(ob.ju[j], ob.ru, ob.jv[j] * ob.rv);
        }
        if (a < 0) continue;
        for (int e = 0; e < 21; ++e) o->U[a][e] = tree(part[e]);
        for (int j = 0; j < 6; ++j) o->gc[a][j] = tree(part[21 + j]);
    }
    memset(part[0], 0, sizeof part[0]);
    for (int i = 0; i < n; ++i)
        if (used[i]) part[0][i % NP] = part[0][i % NP] + o->c[i];
    o->cost = tree(part[0]);
    if (bad) o->cost = INFINITY;
}

/* S24's Cholesky of the 3 x 3 with the damped diagonal; H holds j <= k row-major; L row-major 3 x 3 */
static int chol3(const double* H, double lam, double L[3][3])
{
    static const int at[3][3] = {{0, 1, 2}, {1, 3, 4}, {2, 4, 5}};
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
    return 1;
}

/* L L^T x = b in S24's order */
static void solve3(double L[3][3], const double* b, double* x)
{
    double y[3];
    for (int i = 0; i < 3; ++i) {
        double v = b[i];
        for (int q = 0; q < i; ++q) v = fma(-L[i][q], y[q], v);
        y[i] = v / L[i][i];
    }
    for (int i = 2; i >= 0; --i) {
        double v = y[i];
        for (int q = i + 1; q < 3; ++q) v = fma(-L[q][i], x[q], v);
        x[i] = v / L[i][i];
    }
}

/* S40's Cayley update */
static void update(const double* Rt, const double* d, double* out)
{
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double cc = (h0 * h0 + h1 * h1) + h2 * h2;
    const double s = 1.0 / (1.0 + cc), m = 1.0 - cc;
    double C[9];
    C[0] = (m + 2.0 * (h0 * h0)) * s; C[1] = (2.0 * (h0 * h1 - h2)) * s; C[2] = (2.0 * (h0 * h2 + h1)) * s;
    C[3] = (2.0 * (h0 * h1 + h2)) * s; C[4] = (m + 2.0 * (h1 * h1)) * s; C[5] = (2.0 * (h1 * h2 - h0)) * s;
    C[6] = (2.0 * (h0 * h2 - h1)) * s; C[7] = (2.0 * (h1 * h2 + h0)) * s; C[8] = (m + 2.0 * (h2 * h2)) * s;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (C[3 * r] * Rt[c] + C[3 * r + 1] * Rt[3 + c]) + C[3 * r + 2] * Rt[6 + c];
    for (int i = 0; i < 3; ++i) out[9 + i] = Rt[9 + i] + d[3 + i];
}

static void lin_alloc(Lin* l, int n, int F)
{
    const size_t m = n > 0 ? (size_t)n : 1;
    l->Vp = calloc(m * 6, 8); l->gp = calloc(m * 3, 8); l->c = calloc(m, 8); l->W = calloc(m * F * 18, 8);
}

static void lin_free(Lin* l) { free(l->Vp); free(l->gp); free(l->c); free(l->W); }

/* The whole call over n points (the count already clamped).  K = (fx, fy, cx, cy).  Rt_out: nv x 12; xyz: n x 3, read and
 * written; used (may be NULL): n bytes; cost: (cost_in, cost_out); info: (n_points, n_obs, iters, accepted, status); xyz64
 * (may be NULL): the final fp64 points, n x 3 (the f32 row's value where the point is not used).  Rt_out may alias Rt. */
void ba_run(const double* K, const float* const* uv, const double* const* Rt, int nv, int n, double gate_px, int max_iters,
            unsigned fixed_mask, double* Rt_out, float* xyz, uint8_t* used_out, double* cost, int32_t* info, double* xyz64)
{
    double Pin[MAXV][12], Pc[MAXV][12], Pt[MAXV][12];
    int fidx[MAXV], fview[MAXV], F = 0;
    for (int v = 0; v < nv; ++v) {
        for (int j = 0; j < 12; ++j) Pin[v][j] = Rt[v] ? Rt[v][j] : ((j < 9 && j % 4 == 0) ? 1.0 : 0.0);
        memcpy(Pc[v], Pin[v], sizeof Pin[v]);
        memcpy(Pt[v], Pin[v], sizeof Pin[v]);
        fidx[v] = -1;
        if (!((fixed_mask >> v) & 1u)) { fidx[v] = F; fview[F++] = v; }
    }
    const int M = 6 * F;
    const size_t m = n > 0 ? (size_t)n : 1;
    uint8_t* used = calloc(m, 1);
    double *Xc = calloc(m * 3, 8), *Xt = calloc(m * 3, 8), *Yw = calloc(m * F * 18, 8);
    Lin lin[2];
    lin_alloc(&lin[0], n, F);
    lin_alloc(&lin[1], n, F);

    /* ---- S113: the used set */
    const double g2 = gate_px * gate_px;
    int n_points = 0, n_obs = 0, per_view[MAXV] = {0};
    for (int i = 0; i < n; ++i) {
        int fin = 1;
        for (int c = 0; c < 3; ++c) {
            Xc[3 * i + c] = (double)xyz[3 * i + c];
            fin = fin && fabs(Xc[3 * i + c]) < INFINITY;
        }
        unsigned bits = 0;
        int cnt = 0;
        for (int v = 0; v < nv && fin; ++v) {
            const float x = norm1(uv[v][2 * i], K[2], K[0]), y = norm1(uv[v][2 * i + 1], K[3], K[1]);
            if (!(x == x && y == y)) continue;
            Obs ob;
            observe(K, Pin[v], Xc + 3 * i, uv[v] + 2 * i, &ob);
            if (!ob.depth_ok) continue;
            if (gate_px > 0.0 && !(ob.e <= g2)) continue;
            bits |= 1u << v;
            ++cnt;
        }
        if (cnt < 2) bits = 0;
        used[i] = (uint8_t)bits;
        if (bits) {
            ++n_points;
            n_obs += cnt;
            for (int v = 0; v < nv; ++v) per_view[v] += (bits >> v) & 1;
        }
    }
    int status2 = n_points == 0;
    for (int a = 0; a < F; ++a) status2 = status2 || per_view[fview[a]] < 4;

    int cur_l = 0, iters = 0, accepted = 0;
    linearise(K, uv, Pc, Xc, used, n, nv, fidx, F, &lin[0]);
    const double cost_in = lin[0].cost;
    double cur = cost_in;

    if (!status2 && max_iters > 0) {
        static double part[42][NP];
        static double S[MAXM][MAXM];
        double rhs[MAXM], y[MAXM], d[MAXM];
        double lam = 1e-3;
        for (int it = 0; it < max_iters; ++it) {
            Lin* L0 = &lin[cur_l];
            /* ---- S115 steps 1-2: the damped point blocks and Y = W Vp*^-1 */
            int fail = 0;
            for (int i = 0; i < n; ++i) {
                if (!used[i]) continue;
                double L[3][3];
                if (!chol3(L0->Vp + 6 * i, lam, L)) { fail = 1; continue; }
                for (int a = 0; a < F; ++a) {
                    if (!((used[i] >> fview[a]) & 1)) continue;
                    const double* W = L0->W + ((size_t)i * F + a) * 18;
                    double* Y = Yw + ((size_t)i * F + a) * 18;
                    for (int j = 0; j < 6; ++j) solve3(L, W + 3 * j, Y + 3 * j);
                }
            }
            if (fail) break;
            /* ---- step 3: the reduced system, one pair of free views at a time */
            for (int a = 0; a < F; ++a)
                for (int b = a; b < F; ++b) {
                    memset(part, 0, sizeof part);
                    for (int i = 0; i < n; ++i) {
                        if (!((used[i] >> fview[a]) & (used[i] >> fview[b]) & 1)) continue;
                        const double* Y = Yw + ((size_t)i * F + a) * 18;
                        const double* W = L0->W + ((size_t)i * F + b) * 18;
                        const int p = i % NP;
                        for (int j = 0; j < 6; ++j)
                            for (int k = 0; k < 6; ++k)
                                part[6 * j + k][p] = part[6 * j + k][p] +
                                                     fma(Y[3 * j + 2], W[3 * k + 2], fma(Y[3 * j + 1], W[3 * k + 1], Y[3 * j] * W[3 * k]));
                        if (a != b) continue;
                        const double* g = L0->gp + 3 * i;
                        for (int j = 0; j < 6; ++j)
                            part[36 + j][p] = part[36 + j][p] + fma(Y[3 * j + 2], g[2], fma(Y[3 * j + 1], g[1], Y[3 * j] * g[0]));
                    }
                    if (a == b) {
                        int e = 0;
                        for (int j = 0; j < 6; ++j)
                            for (int k = j; k < 6; ++k, ++e) {
                                const double u = L0->U[a][e];
                                S[6 * a + j][6 * a + k] = (j == k ? u + lam * u : u) - tree(part[6 * j + k]);
                            }
                        for (int j = 0; j < 6; ++j) rhs[6 * a + j] = tree(part[36 + j]) - L0->gc[a][j];
                    } else {
                        for (int j = 0; j < 6; ++j)
                            for (int k = 0; k < 6; ++k) S[6 * a + j][6 * b + k] = -tree(part[6 * j + k]);
                    }
                }
            /* ---- step 4: Cholesky of S (upper entries hold A, lower and diagonal receive L), forward, back */
            for (int j = 0; j < M && !fail; ++j) {
                double dd = S[j][j];
                for (int q = 0; q < j; ++q) dd = fma(-S[j][q], S[j][q], dd);
                if (!(dd > 0.0) || !(dd < INFINITY)) { fail = 1; break; }
                S[j][j] = sqrt(dd);
                for (int i = j + 1; i < M; ++i) {
                    double v = S[j][i];
                    for (int q = 0; q < j; ++q) v = fma(-S[i][q], S[j][q], v);
                    S[i][j] = v / S[j][j];
                }
            }
            if (fail) break;
            for (int i = 0; i < M; ++i) {
                double v = rhs[i];
                for (int q = 0; q < i; ++q) v = fma(-S[i][q], y[q], v);
                y[i] = v / S[i][i];
            }
            for (int i = M - 1; i >= 0; --i) {
                double v = y[i];
                for (int q = i + 1; q < M; ++q) v = fma(-S[q][i], d[q], v);
                d[i] = v / S[i][i];
            }
            /* ---- steps 5-6: the point steps and the step test */
            double dmax = 0.0, hmax = 1.0;
            int fin = 1;
            for (int q = 0; q < M; ++q) {
                const double a = fabs(d[q]);
                if (!(a < INFINITY)) fin = 0;
                if (a > dmax) dmax = a;
            }
            for (int a = 0; a < F; ++a)
                for (int c = 0; c < 3; ++c)
                    if (fabs(Pc[fview[a]][9 + c]) > hmax) hmax = fabs(Pc[fview[a]][9 + c]);
            for (int i = 0; i < n; ++i) {
                if (!used[i]) continue;
                double L[3][3], r[3], dp[3];
                chol3(L0->Vp + 6 * i, lam, L);
                for (int k = 0; k < 3; ++k) r[k] = -L0->gp[3 * i + k];
                for (int a = 0; a < F; ++a) {
                    if (!((used[i] >> fview[a]) & 1)) continue;
                    const double* W = L0->W + ((size_t)i * F + a) * 18;
                    for (int j = 0; j < 6; ++j)
                        for (int k = 0; k < 3; ++k) r[k] = fma(-W[3 * j + k], d[6 * a + j], r[k]);
                }
                solve3(L, r, dp);
                for (int k = 0; k < 3; ++k) {
                    const double a = fabs(dp[k]), x = fabs(Xc[3 * i + k]);
                    if (!(a < INFINITY)) fin = 0;
                    if (a > dmax) dmax = a;
                    if (x > hmax) hmax = x;
                    Xt[3 * i + k] = Xc[3 * i + k] + dp[k];
                }
            }
            if (!fin || !(dmax > 1e-15 * hmax)) break;
            /* ---- steps 7-9 */
            for (int a = 0; a < F; ++a) update(Pc[fview[a]], d + 6 * a, Pt[fview[a]]);
            linearise(K, uv, Pt, Xt, used, n, nv, fidx, F, &lin[1 - cur_l]);
            ++iters;
            if (lin[1 - cur_l].cost < cur) {
                cur = lin[1 - cur_l].cost;
                cur_l = 1 - cur_l;
                lam = lam / 10.0;
                ++accepted;
                for (int a = 0; a < F; ++a) memcpy(Pc[fview[a]], Pt[fview[a]], sizeof Pc[0]);
                double* t = Xc; Xc = Xt; Xt = t;       /* rows of unused points are never read */
            } else {
                lam = lam * 10.0;
            }
        }
    }

    /* ---- S117: result */
    for (int v = 0; v < nv; ++v)
        for (int j = 0; j < 12; ++j) Rt_out[12 * v + j] = (accepted && fidx[v] >= 0) ? Pc[v][j] : Pin[v][j];
    for (int i = 0; i < n; ++i) {
        if (xyz64)
            for (int c = 0; c < 3; ++c) xyz64[3 * i + c] = (accepted && used[i]) ? Xc[3 * i + c] : (double)xyz[3 * i + c];
        if (accepted && used[i])
            for (int c = 0; c < 3; ++c) xyz[3 * i + c] = (float)Xc[3 * i + c];
        if (used_out) used_out[i] = used[i];
    }
    cost[0] = cost_in;
    cost[1] = accepted ? cur : cost_in;
    info[0] = n_points; info[1] = n_obs; info[2] = iters; info[3] = accepted; info[4] = status2 ? 2 : (accepted ? 0 : 1);
    free(used); free(Xc); free(Xt); free(Yw);
    lin_free(&lin[0]);
    lin_free(&lin[1]);
}
