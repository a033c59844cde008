/* pgo_ref.c — plain-C restatement of docs/SPEC.md S118-S123 (pose-graph optimisation over SE(3) / Sim(3) nodes: the used
 * set, the edge residual and its analytic blocks, the linearisation, the Levenberg-Marquardt step solved by block-Jacobi
 * preconditioned conjugate gradients, the result; and the map-point move that follows it).  Built by tests/cref.py with
 * -ffp-contract=off; the only fused multiply-adds are the fma() calls of libm, so the device kernel reproduces these bits.
 * Sums over nodes and over edges keep S23's 512 partials and stride-halving tree; a node's sums run over its used edges in
 * ascending edge id. */
#include <math.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#define NP 512
#define MAXP 7

/* S23's tree over the 512 partials */
static double tree(double* part)
{
    for (int s = NP / 2; s >= 1; s >>= 1)
        for (int p = 0; p < s; ++p) part[p] = part[p] + part[p + s];
    return part[0];
}

/* S119: residual r (P), blocks Ja, Jb (P x P, row-major, row = residual component) of one edge; P = 7 (SIM3) or 6 (RIGID).
 * Returns den > 2^-10. */
static int edge_eval(int P, const double* A, const double* B, const double* Z, const double* w, double* r, double* Ja, double* Jb)
{
    const double *ta = A + 9, *tb = B + 9, *tz = Z + 9;
    const double wr = w[0], wt = w[1], ws = w[2];
    double RD[9], Er[9], u[3], m[3], g[3];
    for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) RD[3 * i + c] = (B[3 * i] * A[3 * c] + B[3 * i + 1] * A[3 * c + 1]) + B[3 * i + 2] * A[3 * c + 2];
    const double sD = B[12] / A[12];
    for (int i = 0; i < 3; ++i) {
        u[i] = (RD[3 * i] * ta[0] + RD[3 * i + 1] * ta[1]) + RD[3 * i + 2] * ta[2];
        m[i] = sD * u[i];
    }
    for (int i = 0; i < 3; ++i)
        for (int c = 0; c < 3; ++c) Er[3 * i + c] = (Z[i] * RD[c] + Z[3 + i] * RD[3 + c]) + Z[6 + i] * RD[6 + c];
    const double den = 1.0 + ((Er[0] + Er[4]) + Er[8]);
    const double id = 1.0 / den;
    g[0] = (Er[7] - Er[5]) * id; g[1] = (Er[2] - Er[6]) * id; g[2] = (Er[3] - Er[1]) * id;
    for (int k = 0; k < 3; ++k) {
        r[k] = wr * (2.0 * g[k]);
        r[3 + k] = wt * ((tb[k] - m[k]) - tz[k]);
    }
    double c = 0.0;
    if (P == 7) {
        const double sigma = sD / Z[12];
        const double is = 1.0 / sigma;
        r[6] = ws * (0.5 * (sigma - is));
        c = 0.5 * (sigma + is);
    }
    for (int e = 0; e < P * P; ++e) Ja[e] = Jb[e] = 0.0;
    /* rotation rows: [g]x = (0, -g2, g1; g2, 0, -g0; -g1, g0, 0) */
    const double X[9] = {0.0, -g[2], g[1], g[2], 0.0, -g[0], -g[1], g[0], 0.0};
    double Mb[9];
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k) {
            const double base = (i == k ? 1.0 : 0.0) + g[i] * g[k];
            Ja[P * i + k] = -(wr * (base + X[3 * i + k]));
            Mb[3 * i + k] = base - X[3 * i + k];
        }
    for (int i = 0; i < 3; ++i)
        for (int k = 0; k < 3; ++k)
            Jb[P * i + k] = wr * ((Mb[3 * i] * Z[3 * k] + Mb[3 * i + 1] * Z[3 * k + 1]) + Mb[3 * i + 2] * Z[3 * k + 2]);
    /* translation rows */
    for (int i = 0; i < 3; ++i) {
        const double q0 = wt * (sD * RD[3 * i]), q1 = wt * (sD * RD[3 * i + 1]), q2 = wt * (sD * RD[3 * i + 2]);
        double* ja = Ja + P * (3 + i);
        ja[0] = -(q1 * ta[2] - q2 * ta[1]);
        ja[1] = -(q2 * ta[0] - q0 * ta[2]);
        ja[2] = -(q0 * ta[1] - q1 * ta[0]);
        ja[3] = -q0; ja[4] = -q1; ja[5] = -q2;
        Jb[P * (3 + i) + 3 + i] = wt;
    }
    const double wm0 = wt * m[0], wm1 = wt * m[1], wm2 = wt * m[2];
    Jb[P * 3 + 1] = -wm2; Jb[P * 3 + 2] = wm1;
    Jb[P * 4 + 0] = wm2;  Jb[P * 4 + 2] = -wm0;
    Jb[P * 5 + 0] = -wm1; Jb[P * 5 + 1] = wm0;
    if (P == 7) {
        Ja[P * 3 + 6] = wm0; Ja[P * 4 + 6] = wm1; Ja[P * 5 + 6] = wm2;
        Jb[P * 3 + 6] = -wm0; Jb[P * 4 + 6] = -wm1; Jb[P * 5 + 6] = -wm2;
        Ja[P * 6 + 6] = -(ws * c);
        Jb[P * 6 + 6] = ws * c;
    }
    return den > 0.0009765625;
}

/* for the tests: one edge's residual and blocks; model 1 = SIM3, 0 = RIGID */
int pgo_edge(int model, const double* A, const double* B, const double* Z, const double* w, double* r, double* Ja, double* Jb)
{
    return edge_eval(model == 1 ? 7 : 6, A, B, Z, w, r, Ja, Jb);
}

static int all_finite(const double* v, int n)
{
    for (int i = 0; i < n; ++i)
        if (!(fabs(v[i]) < INFINITY)) return 0;
    return 1;
}

/* S24's factor of the P x P block with the damped diagonal; D packed j <= k row-major; L row-major 7 x 7 */
static int factor(int P, const double* D, double lam, double L[MAXP][MAXP])
{
    for (int j = 0; j < P; ++j) {
        const double ajj = D[j * P - j * (j - 1) / 2];
        double dd = ajj + lam * ajj;
        for (int k = 0; k < j; ++k) dd = fma(-L[j][k], L[j][k], dd);
        if (!(dd > 0.0) || !(dd < INFINITY)) return 0;
        L[j][j] = sqrt(dd);
        for (int i = j + 1; i < P; ++i) {
            double v = D[j * P - j * (j - 1) / 2 + (i - j)];
            for (int k = 0; k < j; ++k) v = fma(-L[i][k], L[j][k], v);
            L[i][j] = v / L[j][j];
        }
    }
    return 1;
}

static void subst(int P, double L[MAXP][MAXP], const double* b, double* x)
{
    double y[MAXP];
    for (int i = 0; i < P; ++i) {
        double v = b[i];
        for (int k = 0; k < i; ++k) v = fma(-L[i][k], y[k], v);
        y[i] = v / L[i][i];
    }
    for (int i = P - 1; i >= 0; --i) {
        double v = y[i];
        for (int k = i + 1; k < P; ++k) v = fma(-L[k][i], x[k], v);
        x[i] = v / L[i][i];
    }
}

/* S40's Cayley update of R and t; the scale is copied */
static void update(const double* T, const double* d, double* out)
{
    const double h0 = 0.5 * d[0], h1 = 0.5 * d[1], h2 = 0.5 * d[2];
    const double cc = (h0 * h0 + h1 * h1) + h2 * h2;
    const double s = 1.0 / (1.0 + cc), m = 1.0 - cc;
    double C[9];
    C[0] = (m + 2.0 * (h0 * h0)) * s; C[1] = (2.0 * (h0 * h1 - h2)) * s; C[2] = (2.0 * (h0 * h2 + h1)) * s;
    C[3] = (2.0 * (h0 * h1 + h2)) * s; C[4] = (m + 2.0 * (h1 * h1)) * s; C[5] = (2.0 * (h1 * h2 - h0)) * s;
    C[6] = (2.0 * (h0 * h2 - h1)) * s; C[7] = (2.0 * (h1 * h2 + h0)) * s; C[8] = (m + 2.0 * (h2 * h2)) * s;
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) out[3 * r + c] = (C[3 * r] * T[c] + C[3 * r + 1] * T[3 + c]) + C[3 * r + 2] * T[6 + c];
    for (int i = 0; i < 3; ++i) out[9 + i] = T[9 + i] + d[3 + i];
    out[12] = T[12];
}

typedef struct {
    int P, N, E;
    const int32_t* ab;
    const double *Z, *w;
    const uint8_t* used;
    const uint8_t* fre;
    const int *start, *inc;      /* incidence: node i's entries inc[start[i] .. start[i+1]), entry = 2 e + side */
} Graph;

typedef struct {
    double *r, *Ja, *Jb;         /* per edge: P, P*P, P*P */
    double *D, *g;               /* per node: P(P+1)/2, P */
    double cost;
} Lin;

/* S120: the linearisation at the poses T; bad: a trial scale already failed */
static void linearise(const Graph* G, const double* T, int bad, Lin* o)
{
    static double part[NP];
    const int P = G->P, TRI = P * (P + 1) / 2;
    memset(part, 0, sizeof part);
    for (int e = 0; e < G->E; ++e) {
        if (!G->used[e]) continue;
        double* r = o->r + (size_t)P * e;
        if (!edge_eval(P, T + 13 * G->ab[2 * e], T + 13 * G->ab[2 * e + 1], G->Z + 13 * (size_t)e, G->w + 3 * (size_t)e, r,
                       o->Ja + (size_t)P * P * e, o->Jb + (size_t)P * P * e))
            bad = 1;
        double c = 0.0;
        for (int k = 0; k < P; ++k) c = fma(r[k], r[k], c);
        part[e % NP] = part[e % NP] + c;
    }
    o->cost = tree(part);
    if (bad) o->cost = INFINITY;
    for (int i = 0; i < G->N; ++i) {
        if (!G->fre[i]) continue;
        double* D = o->D + (size_t)TRI * i;
        double* g = o->g + (size_t)P * i;
        for (int k = 0; k < TRI; ++k) D[k] = 0.0;
        for (int k = 0; k < P; ++k) g[k] = 0.0;
        for (int q = G->start[i]; q < G->start[i + 1]; ++q) {
            const int e = G->inc[q] >> 1;
            const double* J = ((G->inc[q] & 1) ? o->Jb : o->Ja) + (size_t)P * P * e;
            const double* r = o->r + (size_t)P * e;
            for (int row = 0; row < P; ++row) {
                int k = 0;
                for (int j = 0; j < P; ++j)
                    for (int c = j; c < P; ++c, ++k) D[k] = fma(J[P * row + j], J[P * row + c], D[k]);
                for (int j = 0; j < P; ++j) g[j] = fma(J[P * row + j], r[row], g[j]);
            }
        }
    }
}

static void lin_alloc(Lin* l, int P, int N, int E)
{
    const size_t n = N > 0 ? N : 1, e = E > 0 ? E : 1;
    l->r = calloc(e * P, 8); l->Ja = calloc(e * P * P, 8); l->Jb = calloc(e * P * P, 8);
    l->D = calloc(n * (P * (P + 1) / 2), 8); l->g = calloc(n * P, 8);
}

static void lin_free(Lin* l) { free(l->r); free(l->Ja); free(l->Jb); free(l->D); free(l->g); }

/* S23 sum over the free nodes of the dot product of two node vectors: t = a_0 b_0, t = fma(a_j, b_j, t) */
static double node_dot(const Graph* G, const double* a, const double* b)
{
    static double part[NP];
    memset(part, 0, sizeof part);
    for (int i = 0; i < G->N; ++i) {
        if (!G->fre[i]) continue;
        const double *x = a + (size_t)G->P * i, *y = b + (size_t)G->P * i;
        double t = x[0] * y[0];
        for (int j = 1; j < G->P; ++j) t = fma(x[j], y[j], t);
        part[i % NP] = part[i % NP] + t;
    }
    return tree(part);
}

/* The whole call over E edges (the count already clamped).  model 1 = SIM3, 0 = RIGID.  pose_out may alias pose_in.
 * cost: (cost_in, cost_out); info: (n_edges_used, n_nodes_free, iters, accepted, cg_total, status). */
void pgo_run(int model, const double* pose_in, int N, const uint8_t* fixed, const int32_t* ab, const double* Z, const double* w, int E,
             int max_iters, int cg_iters, double cg_tol, double* pose_out, uint8_t* used_out, double* cost, int32_t* info)
{
    const int P = model == 1 ? 7 : 6, TRI = P * (P + 1) / 2;
    const size_t n1 = N > 0 ? N : 1, e1 = E > 0 ? E : 1;
    double *Tc = malloc(n1 * 13 * 8), *Tt = malloc(n1 * 13 * 8);
    memcpy(Tc, pose_in, (size_t)N * 13 * 8);
    memcpy(Tt, pose_in, (size_t)N * 13 * 8);
    uint8_t *used = calloc(e1, 1), *fre = calloc(n1, 1);
    int *start = calloc(n1 + 1, sizeof(int)), *inc = calloc(2 * e1, sizeof(int)), *cur = calloc(n1, sizeof(int));

    /* ---- S118: the used set, the incidence lists, the free nodes */
    int n_used = 0, n_free = 0, n_fixed = 0;
    for (int e = 0; e < E; ++e) {
        const int a = ab[2 * e], b = ab[2 * e + 1];
        if (a < 0 || a >= N || b < 0 || b >= N || a == b) continue;
        const double *A = Tc + 13 * a, *B = Tc + 13 * b, *Ze = Z + 13 * (size_t)e, *we = w + 3 * (size_t)e;
        if (!all_finite(Ze, 13) || !all_finite(we, 3) || !all_finite(A, 13) || !all_finite(B, 13)) continue;
        if (!(Ze[12] > 0.0) || !(A[12] > 0.0) || !(B[12] > 0.0)) continue;
        if (fixed[a] && fixed[b]) continue;
        double r[MAXP], Ja[MAXP * MAXP], Jb[MAXP * MAXP];
        if (!edge_eval(P, A, B, Ze, we, r, Ja, Jb)) continue;
        used[e] = 1;
        ++n_used;
        ++start[a + 1];
        ++start[b + 1];
    }
    for (int i = 0; i < N; ++i) {
        fre[i] = !fixed[i] && start[i + 1] > 0;
        n_free += fre[i];
        n_fixed += fixed[i] != 0;
        start[i + 1] += start[i];
        cur[i] = start[i];
    }
    for (int e = 0; e < E; ++e)
        if (used[e]) {
            inc[cur[ab[2 * e]]++] = 2 * e;
            inc[cur[ab[2 * e + 1]]++] = 2 * e + 1;
        }
    const int status2 = n_used == 0 || n_fixed == 0;
    const Graph G = {P, N, E, ab, Z, w, used, fre, start, inc};

    Lin lin[2];
    lin_alloc(&lin[0], P, N, E);
    lin_alloc(&lin[1], P, N, E);
    double *Lf = calloc(n1 * MAXP * MAXP, 8), *x = calloc(n1 * P, 8), *rr = calloc(n1 * P, 8), *z = calloc(n1 * P, 8);
    double *p = calloc(n1 * P, 8), *Ap = calloc(n1 * P, 8), *q = calloc(e1 * P, 8);

    int cl = 0, iters = 0, accepted = 0, cg_total = 0;
    linearise(&G, Tc, 0, &lin[0]);
    const double cost_in = lin[0].cost;
    double cur_cost = cost_in;

    if (!status2 && max_iters > 0) {
        double lam = 1e-3;
        for (int it = 0; it < max_iters; ++it) {
            const Lin* L0 = &lin[cl];
            /* ---- S121 step 1: the damped diagonal blocks */
            int fail = 0;
            for (int i = 0; i < N; ++i)
                if (fre[i] && !factor(P, L0->D + (size_t)TRI * i, lam, (double(*)[MAXP])(Lf + (size_t)MAXP * MAXP * i))) fail = 1;
            if (fail) break;
            /* ---- step 2: PCG from x = 0 */
            for (int i = 0; i < N; ++i) {
                if (!fre[i]) continue;
                for (int j = 0; j < P; ++j) {
                    x[(size_t)P * i + j] = 0.0;
                    rr[(size_t)P * i + j] = -L0->g[(size_t)P * i + j];
                }
                subst(P, (double(*)[MAXP])(Lf + (size_t)MAXP * MAXP * i), rr + (size_t)P * i, z + (size_t)P * i);
                for (int j = 0; j < P; ++j) p[(size_t)P * i + j] = z[(size_t)P * i + j];
            }
            double rho = node_dot(&G, rr, z);
            const double rho0 = rho;
            int stop = 0;
            for (int k = 0; k < cg_iters; ++k) {
                for (int e = 0; e < E; ++e) {
                    if (!used[e]) continue;
                    const int a = ab[2 * e], b = ab[2 * e + 1];
                    for (int row = 0; row < P; ++row) {
                        double v = 0.0;
                        if (fre[a])
                            for (int j = 0; j < P; ++j) v = fma(L0->Ja[(size_t)P * P * e + P * row + j], p[(size_t)P * a + j], v);
                        if (fre[b])
                            for (int j = 0; j < P; ++j) v = fma(L0->Jb[(size_t)P * P * e + P * row + j], p[(size_t)P * b + j], v);
                        q[(size_t)P * e + row] = v;
                    }
                }
                for (int i = 0; i < N; ++i) {
                    if (!fre[i]) continue;
                    double acc[MAXP] = {0};
                    for (int s = start[i]; s < start[i + 1]; ++s) {
                        const int e = inc[s] >> 1;
                        const double* J = ((inc[s] & 1) ? L0->Jb : L0->Ja) + (size_t)P * P * e;
                        for (int row = 0; row < P; ++row)
                            for (int j = 0; j < P; ++j) acc[j] = fma(J[P * row + j], q[(size_t)P * e + row], acc[j]);
                    }
                    for (int j = 0; j < P; ++j)
                        Ap[(size_t)P * i + j] = acc[j] + (lam * L0->D[(size_t)TRI * i + j * P - j * (j - 1) / 2]) * p[(size_t)P * i + j];
                }
                const double pAp = node_dot(&G, p, Ap);
                if (!(pAp > 0.0) || !(pAp < INFINITY)) {
                    if (k == 0) stop = 1;
                    break;
                }
                const double alpha = rho / pAp;
                for (int i = 0; i < N; ++i) {
                    if (!fre[i]) continue;
                    for (int j = 0; j < P; ++j) {
                        x[(size_t)P * i + j] = fma(alpha, p[(size_t)P * i + j], x[(size_t)P * i + j]);
                        rr[(size_t)P * i + j] = fma(-alpha, Ap[(size_t)P * i + j], rr[(size_t)P * i + j]);
                    }
                    subst(P, (double(*)[MAXP])(Lf + (size_t)MAXP * MAXP * i), rr + (size_t)P * i, z + (size_t)P * i);
                }
                const double rho1 = node_dot(&G, rr, z);
                ++cg_total;
                if (rho1 <= (cg_tol * cg_tol) * rho0) break;
                if (k + 1 == cg_iters) break;
                const double beta = rho1 / rho;
                for (int i = 0; i < N; ++i) {
                    if (!fre[i]) continue;
                    for (int j = 0; j < P; ++j) p[(size_t)P * i + j] = fma(beta, p[(size_t)P * i + j], z[(size_t)P * i + j]);
                }
                rho = rho1;
            }
            if (stop) break;
            /* ---- step 5: the step test */
            double dmax = 0.0, hmax = 1.0;
            int fin = 1;
            for (int i = 0; i < N; ++i) {
                if (!fre[i]) continue;
                for (int j = 0; j < P; ++j) {
                    const double a = fabs(x[(size_t)P * i + j]);
                    if (!(a < INFINITY)) fin = 0;
                    if (a > dmax) dmax = a;
                }
                for (int c = 0; c < 3; ++c)
                    if (fabs(Tc[13 * i + 9 + c]) > hmax) hmax = fabs(Tc[13 * i + 9 + c]);
            }
            if (!fin || !(dmax > 1e-15 * hmax)) break;
            /* ---- step 6: the trial */
            int bad = 0;
            for (int i = 0; i < N; ++i) {
                if (!fre[i]) continue;
                update(Tc + 13 * i, x + (size_t)P * i, Tt + 13 * i);
                if (P == 7) {
                    const double s = Tc[13 * i + 12] * (1.0 + x[(size_t)P * i + 6]);
                    Tt[13 * i + 12] = s;
                    if (!(s > 0.0) || !(s < INFINITY)) bad = 1;
                }
            }
            linearise(&G, Tt, bad, &lin[1 - cl]);
            ++iters;
            if (lin[1 - cl].cost < cur_cost) {
                cur_cost = lin[1 - cl].cost;
                cl = 1 - cl;
                lam = lam / 10.0;
                ++accepted;
                double* t = Tc; Tc = Tt; Tt = t;      /* held nodes are equal in both */
            } else {
                lam = lam * 10.0;
            }
        }
    }

    /* ---- S122: result.  Tc is the input until a step is accepted, and held nodes never change in it */
    memmove(pose_out, Tc, (size_t)N * 13 * 8);
    if (used_out) memcpy(used_out, used, (size_t)E);
    cost[0] = cost_in;
    cost[1] = accepted ? cur_cost : cost_in;
    info[0] = n_used; info[1] = n_free; info[2] = iters; info[3] = accepted; info[4] = cg_total;
    info[5] = status2 ? 2 : (accepted ? 0 : 1);
    free(Tc); free(Tt); free(used); free(fre); free(start); free(inc); free(cur);
    free(Lf); free(x); free(rr); free(z); free(p); free(Ap); free(q);
    lin_free(&lin[0]);
    lin_free(&lin[1]);
}

/* S123: out[i] = (float)(P_new,k^-1 (P_old,k X_i)), k = anchor[i]; fp64, one rounding; NaN rows */
void pgo_move(const double* Told, const double* Tnew, int N, const int32_t* anchor, const float* xyz, int n, float* out)
{
    for (int i = 0; i < n; ++i) {
        const int k = anchor[i];
        const double X[3] = {(double)xyz[3 * i], (double)xyz[3 * i + 1], (double)xyz[3 * i + 2]};
        int fin = k >= 0 && k < N && all_finite(X, 3);
        double o[3] = {0.0, 0.0, 0.0};
        if (fin) {
            const double *A = Told + 13 * (size_t)k, *B = Tnew + 13 * (size_t)k;
            fin = all_finite(A, 13) && all_finite(B, 13);
            double v[3];
            for (int r = 0; r < 3; ++r)
                v[r] = ((((A[12] * A[3 * r]) * X[0] + (A[12] * A[3 * r + 1]) * X[1]) + (A[12] * A[3 * r + 2]) * X[2]) + A[9 + r]) - B[9 + r];
            for (int c = 0; c < 3; ++c) {
                o[c] = ((B[c] * v[0] + B[3 + c] * v[1]) + B[6 + c] * v[2]) / B[12];
                fin = fin && fabs(o[c]) < INFINITY;
            }
        }
        for (int c = 0; c < 3; ++c) out[3 * i + c] = fin ? (float)o[c] : NAN;
    }
}
