/*
 * relmc_oracle.c — TEST INFRASTRUCTURE ONLY.  CPU restatement (plain C) of the reference's
 * mc_sampling + mc_simulation hot path.  Only tests/, __graft_entry__.smoke() and bench.py's
 * cpu_baseline leg may load this library; the product (include/relmc.h) never does.
 *
 * PARITY PIN.  The arithmetic of the path lives in MATPOWER (runopf -> dcopf_solver -> qps_mips -> mips; call site
 * Montecarlo_nsq_single/mc_simulation.m:41), an un-vendored and un-pinned dependency of the reference (README.md:46-48), and the
 * reference holds no tests and no per-state vectors: no single state's (dns, nodal, iterations) can be compared with the reference's.
 * This file restates MATPOWER's published algorithm on the UNREDUCED formulation — variables [Va; Pg], MIPS'
 * own equality/inequality split, the full (nx+neq) KKT system solved by LU with partial pivoting, as MATLAB's `\` would — so that it
 * is independent of the reduced in-register elimination the HIP kernels use.  What pins it:
 *  (a) per state: scipy/HiGHS LP values and the numpy MIPS of oracle/pyoracle.py (tests/golden/states_fixture.json);
 *  (b) the reference's golden artifacts reliability_results.mat / nodal_results.csv (tests/golden/nsq_golden.json), as joint statistics
 *      of the converged means (tests/golden_stats.py: nodal vector, importance vector, (EDNS, PLC));
 *  (c) round 6 — WHERE THE INTERIOR POINT STOPS, from reference-held data: edns_history / beta_history reconstruct the golden run's
 *      1 000 per-batch sums of dns and dns^2; every batch sum is whole MW plus the sum of MIPS' termination residuals f + 2850 over the
 *      batch's shed samples (2.332e-07 MW per shed sample).  This oracle reproduces that distribution (two-sample KS p = 0.36, mean
 *      residual within 0.02 %), and the same statistic rejects comptol x or / 10, sigma = 0.2, xi = 0.9995, z0 = 2 at p < 1e-70
 *      (tests/test_oracle.py): the recalled MIPS constants and the start point are pinned by the reference's own vectors.  34 golden
 *      batches carry one sample of 1 434 +- 16 MW: the isolated-bus state's dns = load / 2 = 1 425 MW of REFERENCE_EMULATE, read off the
 *      golden histories (PHYSICAL rejected at p = 7e-50).
 *
 * Reference lines followed:
 *   mc_sampling.m:24-41      -> orc_mc_sampling (counter-based RNG instead of rand, strict '<')
 *   mc_simulation.m:32-37    -> status mapping (1 = failed -> component removed)
 *   mc_simulation.m:41       -> solve_state (MATPOWER DC-OPF + MIPS)
 *   mc_simulation.m:54-59    -> dns = f + load, dns < 0.1 -> 0
 *   mc_simulation.m:62-99    -> nodal shed of the virtual generators, > 1e-3
 *   nsqMain.m:270,282-301    -> accumulators (fail flag dns > 1e-4)
 *   nsqMain.m:208-308        -> orc_nsq_database (the loop in its own unique-state database form)
 */
#include "relmc_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

/* ------------------------------------------------------------------------------------ */
/* Philox4x32-10 (Salmon, Moraes, Dror, Shaw: "Parallel random numbers: as easy as 1,2,3") */
/* ------------------------------------------------------------------------------------ */
static void philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    uint32_t c0 = ctr[0], c1 = ctr[1], c2 = ctr[2], c3 = ctr[3];
    uint32_t k0 = key[0], k1 = key[1];
    for (int r = 0; r < 10; ++r) {
        uint64_t p0 = (uint64_t)0xD2511F53u * c0;
        uint64_t p1 = (uint64_t)0xCD9E8D57u * c2;
        uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0;
        uint32_t n1 = (uint32_t)p1;
        uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        uint32_t n3 = (uint32_t)p0;
        c0 = n0; c1 = n1; c2 = n2; c3 = n3;
        k0 += 0x9E3779B9u;
        k1 += 0xBB67AE85u;
    }
    out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

void orc_philox4x32_10(const uint32_t ctr[4], const uint32_t key[2], uint32_t out[4])
{
    philox4x32_10(ctr, key, out);
}

void orc_thresholds(const relmc_case_desc* c, uint32_t* thr)
{
    int ncomp = c->ng + c->nl;
    for (int k = 0; k < ncomp; ++k) {
        double t = floor(c->unavail[k] * 4294967296.0);
        if (t < 0) t = 0;
        if (t > 4294967295.0) t = 4294967295.0;
        thr[k] = c->always_up[k] ? 0u : (uint32_t)t;
    }
}

/* one scenario: component k failed iff philox(ctr=(i_lo,i_hi,k>>2,0), key=seed)[k&3] < thr[k] */
static void sample_state(const uint32_t* thr, int ncomp, uint64_t seed, uint64_t index, uint8_t* st)
{
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int blk = 0; blk * 4 < ncomp; ++blk) {
        uint32_t ctr[4] = {(uint32_t)index, (uint32_t)(index >> 32), (uint32_t)blk, 0u};
        uint32_t r[4];
        philox4x32_10(ctr, key, r);
        for (int e = 0; e < 4 && blk * 4 + e < ncomp; ++e)
            st[blk * 4 + e] = r[e] < thr[blk * 4 + e] ? 1 : 0;
    }
}

int32_t orc_mc_sampling(const relmc_case_desc* c, uint64_t seed, uint64_t first_index, int64_t n,
                        uint8_t* eqstatus)
{
    int ncomp = c->ng + c->nl;
    uint32_t thr[RELMC_MAX_COMP];
    if (ncomp > RELMC_MAX_COMP) return RELMC_ERR_UNSUPPORTED;
    orc_thresholds(c, thr);
    for (int64_t i = 0; i < n; ++i)
        sample_state(thr, ncomp, seed, first_index + (uint64_t)i, eqstatus + i * ncomp);
    return RELMC_OK;
}

/* ------------------------------------------------------------------------------------ */
/* workspace                                                                            */
/* ------------------------------------------------------------------------------------ */
typedef struct {
    int nx_max, neq_max, niq_max, nk_max;
    /* sparse rows of Ae / Ai: each row has at most rw entries */
    int rw;
    int *ae_n, *ae_idx; double *ae_val, *be;
    int *ai_n, *ai_idx; double *ai_val, *bi;
    double *x, *x0, *c, *xmin, *xmax;
    double *lam, *z, *mu, *h, *g, *Lx, *N, *dz, *dmu;
    double *K, *rhs;
    int *piv;
    int *inj_of_col;     /* LP column -> case injection index */
    int *lab, *deg;
    uint8_t *inj_on, *br_on, *pin, *drop;
    double *pmin;
} orc_ws;

static void* xm(size_t n) { void* p = calloc(n ? n : 1, 1); if (!p) abort(); return p; }

static orc_ws* ws_new(const relmc_case_desc* c)
{
    orc_ws* w = (orc_ws*)xm(sizeof(orc_ws));
    int ninj = c->ng + c->nd;
    w->nx_max = c->nb + ninj;
    w->neq_max = 2 * c->nb + ninj;            /* balance + pins + fixed injections */
    w->niq_max = 2 * c->nl + 2 * ninj;
    w->nk_max = w->nx_max + w->neq_max;
    w->rw = c->nb + ninj + 1;
    w->ae_n = xm(sizeof(int) * w->neq_max);
    w->ae_idx = xm(sizeof(int) * (size_t)w->neq_max * w->rw);
    w->ae_val = xm(sizeof(double) * (size_t)w->neq_max * w->rw);
    w->be = xm(sizeof(double) * w->neq_max);
    w->ai_n = xm(sizeof(int) * w->niq_max);
    w->ai_idx = xm(sizeof(int) * (size_t)w->niq_max * 2);
    w->ai_val = xm(sizeof(double) * (size_t)w->niq_max * 2);
    w->bi = xm(sizeof(double) * w->niq_max);
    w->x = xm(sizeof(double) * w->nx_max); w->x0 = xm(sizeof(double) * w->nx_max);
    w->c = xm(sizeof(double) * w->nx_max);
    w->xmin = xm(sizeof(double) * w->nx_max); w->xmax = xm(sizeof(double) * w->nx_max);
    w->lam = xm(sizeof(double) * w->neq_max); w->g = xm(sizeof(double) * w->neq_max);
    w->z = xm(sizeof(double) * w->niq_max); w->mu = xm(sizeof(double) * w->niq_max);
    w->h = xm(sizeof(double) * w->niq_max); w->dz = xm(sizeof(double) * w->niq_max);
    w->dmu = xm(sizeof(double) * w->niq_max);
    w->Lx = xm(sizeof(double) * w->nx_max); w->N = xm(sizeof(double) * w->nx_max);
    w->K = xm(sizeof(double) * (size_t)w->nk_max * w->nk_max);
    w->rhs = xm(sizeof(double) * w->nk_max);
    w->piv = xm(sizeof(int) * w->nk_max);
    w->inj_of_col = xm(sizeof(int) * w->nx_max);
    w->lab = xm(sizeof(int) * c->nb); w->deg = xm(sizeof(int) * c->nb);
    w->inj_on = xm(ninj); w->br_on = xm(c->nl); w->pin = xm(c->nb); w->drop = xm(c->nb);
    w->pmin = xm(sizeof(double) * ninj);
    return w;
}

static void ws_free(orc_ws* w)
{
    free(w->ae_n); free(w->ae_idx); free(w->ae_val); free(w->be);
    free(w->ai_n); free(w->ai_idx); free(w->ai_val); free(w->bi);
    free(w->x); free(w->x0); free(w->c); free(w->xmin); free(w->xmax);
    free(w->lam); free(w->g); free(w->z); free(w->mu); free(w->h); free(w->dz); free(w->dmu);
    free(w->Lx); free(w->N); free(w->K); free(w->rhs); free(w->piv); free(w->inj_of_col);
    free(w->lab); free(w->deg); free(w->inj_on); free(w->br_on); free(w->pin); free(w->drop);
    free(w->pmin); free(w);
}

/* ------------------------------------------------------------------------------------ */
/* dense LU with partial pivoting (what MATLAB's `\` does for a square system)           */
/* returns 0 ok, 1 exactly singular (zero pivot column -> Inf/NaN solution in MATLAB)    */
/* ------------------------------------------------------------------------------------ */
static int lu_solve(double* A, int n, int lda, double* b, int* piv)
{
    for (int k = 0; k < n; ++k) {
        int p = k; double best = fabs(A[k * lda + k]);
        for (int i = k + 1; i < n; ++i) {
            double v = fabs(A[i * lda + k]);
            if (v > best) { best = v; p = i; }
        }
        piv[k] = p;
        if (best == 0.0 || best != best) return 1;
        if (p != k) {
            for (int j = 0; j < n; ++j) { double t = A[k * lda + j]; A[k * lda + j] = A[p * lda + j]; A[p * lda + j] = t; }
            double t = b[k]; b[k] = b[p]; b[p] = t;
        }
        double inv = 1.0 / A[k * lda + k];
        for (int i = k + 1; i < n; ++i) {
            double m = A[i * lda + k];
            if (m == 0.0) continue;
            m *= inv;
            A[i * lda + k] = m;
            double* ri = A + i * lda; const double* rk = A + k * lda;
            for (int j = k + 1; j < n; ++j) ri[j] -= m * rk[j];
            b[i] -= m * b[k];
        }
    }
    for (int i = n - 1; i >= 0; --i) {
        double s = b[i];
        const double* ri = A + i * lda;
        for (int j = i + 1; j < n; ++j) s -= ri[j] * b[j];
        b[i] = s / ri[i];
    }
    return 0;
}

/* ------------------------------------------------------------------------------------ */
/* topology pre-processing (policy rows of SURVEY.md §8a)                                */
/* ------------------------------------------------------------------------------------ */
static int uf_find(int* p, int a) { while (p[a] != a) { p[a] = p[p[a]]; a = p[a]; } return a; }

typedef struct { int singular; int n_relaxed; } pre_info;

static pre_info preprocess(const relmc_case_desc* c, const uint8_t* st, int policy, double scale, orc_ws* w)
{
    pre_info pi = {0, 0};
    int nb = c->nb, ng = c->ng, nl = c->nl, ninj = c->ng + c->nd;
    /* seq_mcsimulation.m:38-39: the virtual generators' Pmin (= -load) is scaled by the hourly load factor */
    for (int j = 0; j < ninj; ++j) { w->inj_on[j] = j < ng ? !st[j] : 1; w->pmin[j] = j < ng ? c->inj_pmin[j] : c->inj_pmin[j] * scale; }
    for (int i = 0; i < nb; ++i) { w->lab[i] = i; w->deg[i] = 0; w->pin[i] = 0; w->drop[i] = 0; }
    for (int l = 0; l < nl; ++l) {
        w->br_on[l] = !st[ng + l];
        if (!w->br_on[l]) continue;
        int f = c->br_from[l], t = c->br_to[l];
        w->deg[f]++; w->deg[t]++;
        int a = uf_find(w->lab, f), b = uf_find(w->lab, t);
        if (a != b) { if (a < b) w->lab[b] = a; else w->lab[a] = b; }
    }
    for (int i = 0; i < nb; ++i) w->lab[i] = uf_find(w->lab, i);   /* label = lowest bus of island */
    if (policy == RELMC_REFERENCE_EMULATE)
        for (int i = 0; i < nb; ++i) if (w->deg[i] == 0) pi.singular = 1;
    if (pi.singular) return pi;   /* never solved: MATPOWER's own start point is returned */
    int ref_lab = w->lab[c->ref_bus];
    for (int root = 0; root < nb; ++root) {
        if (w->lab[root] != root) continue;
        int pin = c->ref_bus;            /* rule 1: reference bus, else the island's highest bus */
        if (root != ref_lab) for (int i = 0; i < nb; ++i) if (w->lab[i] == root) pin = i;
        w->pin[pin] = 1;
        int n_inj = 0, n_load = 0, n_gen = 0, n_free = 0; double lo_sum = 0;
#define IN_ISLAND(j) (w->inj_on[j] && w->lab[c->inj_bus[j]] == root)
        for (int j = 0; j < ninj; ++j)
            if (IN_ISLAND(j)) {
                n_inj++; lo_sum += w->pmin[j];
                if (j >= ng) n_load++; else if (c->inj_pmax[j] > 0) n_gen++;
            }
        if (n_inj && !n_load) {          /* rule 2: island without load: decommit its generators */
            for (int j = 0; j < ng; ++j) if (IN_ISLAND(j)) w->inj_on[j] = 0;
            pi.n_relaxed++;
        } else if (n_load && !n_gen) {   /* rule 3: island without generation: all load shed, p = 0 */
            for (int j = ng; j < ninj; ++j) if (IN_ISLAND(j)) w->pmin[j] = 0.0;
        } else if (lo_sum > 1e-9) {      /* rule 4: over-generation: relax Pmin of the island's units */
            for (int j = 0; j < ng; ++j) if (IN_ISLAND(j)) w->pmin[j] = 0.0;
            pi.n_relaxed++;
        }
        for (int j = 0; j < ninj; ++j) if (IN_ISLAND(j) && c->inj_pmax[j] - w->pmin[j] > 0) n_free++;
        if (!n_free) w->drop[pin] = 1;   /* rule 5: balance rows of the island are dependent */
#undef IN_ISLAND
    }
    return pi;
}

/* ------------------------------------------------------------------------------------ */
/* one state: MATPOWER DC-OPF assembly + MIPS                                            */
/* ------------------------------------------------------------------------------------ */
static void add_ae(orc_ws* w, int row, int idx, double val)
{
    int n = w->ae_n[row]++;
    w->ae_idx[row * w->rw + n] = idx; w->ae_val[row * w->rw + n] = val;
}

static void finish(const relmc_case_desc* c, const orc_ws* w, int ncol, double f, double scale, double* dns_out,
                   double* nodal)
{
    /* mc_simulation.m:54-59 */
    double dns = f + c->total_load * scale;      /* mc_simulation.m:54 / seq_mcsimulation.m:42,67 */
    if (dns < 0.1) dns = 0.0;
    for (int i = 0; i < c->nb; ++i) nodal[i] = 0.0;
    if (dns > 0) {                       /* mc_simulation.m:65 */
        for (int col = 0; col < ncol; ++col) {
            int j = w->inj_of_col[col];
            if (j < c->ng) continue;
            double shed = w->x[c->nb + col] * c->base_mva - c->inj_pmin[j] * scale;   /* Pg - Pmin, :86 */
            if (shed > 1e-3) nodal[c->inj_bus[j]] = shed;                      /* :90-97 */
        }
    }
    *dns_out = dns;
}

static void solve_state(const relmc_case_desc* c, const uint8_t* st, double scale, const relmc_solver_opts* o,
                        orc_ws* w, double* dns, double* nodal, int32_t* status, int32_t* iters,
                        int32_t* relaxed)
{
    const int nb = c->nb, nl = c->nl, ninj = c->ng + c->nd;
    const double base = c->base_mva;
    const double eps = 2.220446049250313e-16;
    pre_info pi = preprocess(c, st, o->singular_policy, scale, w);
    *relaxed = pi.n_relaxed;

    /* ---- variables: x = [Va(nb); Pg of in-service injections] (ext2int drops the rest) */
    int ncol = 0;
    for (int j = 0; j < ninj; ++j) if (w->inj_on[j]) w->inj_of_col[ncol++] = j;
    const int nx = nb + ncol;
    for (int i = 0; i < nb; ++i) {
        w->c[i] = 0.0;
        if (w->pin[i]) { w->xmin[i] = 0.0; w->xmax[i] = 0.0; }
        else { w->xmin[i] = -INFINITY; w->xmax[i] = INFINITY; }
    }
    for (int col = 0; col < ncol; ++col) {
        int j = w->inj_of_col[col];
        w->xmin[nb + col] = w->pmin[j] / base;
        w->xmax[nb + col] = c->inj_pmax[j] / base;
        w->c[nb + col] = c->inj_cost[j] * base;        /* opf_setup: c1 * baseMVA */
    }
    /* dcopf_solver start: midpoint of bounds (Inf -> +-1e10), all angles = ref angle */
    for (int k = 0; k < nx; ++k) {
        double lb = isinf(w->xmin[k]) ? -1e10 : w->xmin[k];
        double ub = isinf(w->xmax[k]) ? 1e10 : w->xmax[k];
        w->x0[k] = k < nb ? 0.0 : (lb + ub) / 2.0;
    }
    if (pi.singular) {
        /* isolated bus: zero KKT column -> MATLAB `\` returns Inf/NaN -> mips breaks in
         * iteration 1 ("numerically failed") and returns x0 */
        double f = 0;
        for (int k = 0; k < nx; ++k) { w->x[k] = w->x0[k]; f += w->c[k] * w->x0[k]; }
        finish(c, w, ncol, f, scale, dns, nodal);
        *status = RELMC_ST_SINGULAR; *iters = 0;
        return;
    }

    /* ---- mips: AA = [I; A], split into equalities / inequalities --------------------- */
    int neq = 0, niq = 0;
    /* variable-bound rows first (AA = [speye(nx); A]) — classified like mips.m:         */
    /* ieq: |uu-ll|<=eps ; ilt: ll<=-1e10 & uu<1e10 ; igt: uu>=1e10 & ll>-1e10 ; ibx      */
    /* Ai = [AA(ilt); -AA(igt); AA(ibx); -AA(ibx)], built in four passes to keep the order */
    /* equalities */
    for (int k = 0; k < nx; ++k)
        if (fabs(w->xmax[k] - w->xmin[k]) <= eps) { w->ae_n[neq] = 0; add_ae(w, neq, k, 1.0); w->be[neq] = w->xmax[k]; neq++; }
    for (int i = 0; i < nb; ++i) {                  /* Pmis rows: Bbus*Va - Cg*Pg = 0 */
        if (w->drop[i]) continue;
        w->ae_n[neq] = 0;
        /* Bbus row i = sum over in-service branches at i (makeBdc) */
        double diag = 0;
        for (int l = 0; l < nl; ++l) {
            if (!w->br_on[l]) continue;
            if (c->br_from[l] == i) { diag += c->br_b[l]; add_ae(w, neq, c->br_to[l], -c->br_b[l]); }
            else if (c->br_to[l] == i) { diag += c->br_b[l]; add_ae(w, neq, c->br_from[l], -c->br_b[l]); }
        }
        if (diag != 0) add_ae(w, neq, i, diag);
        for (int col = 0; col < ncol; ++col)
            if (c->inj_bus[w->inj_of_col[col]] == i) add_ae(w, neq, nb + col, -1.0);
        w->be[neq] = 0.0;
        neq++;
    }
#define ADD_AI(i0, v0, i1, v1, rhs)                                                      \
    do { w->ai_idx[niq * 2] = (i0); w->ai_val[niq * 2] = (v0); w->ai_idx[niq * 2 + 1] = (i1); \
         w->ai_val[niq * 2 + 1] = (v1); w->ai_n[niq] = ((i1) >= 0) ? 2 : 1; w->bi[niq] = (rhs); niq++; } while (0)
    /* pass ilt / igt on variable bounds: none of our variables is one-sided (angles are
     * free or pinned, injections are boxed or fixed); keep the general test anyway */
    for (int k = 0; k < nx; ++k)
        if (w->xmin[k] <= -1e10 && w->xmax[k] < 1e10) ADD_AI(k, 1.0, -1, 0.0, w->xmax[k]);
    for (int k = 0; k < nx; ++k)
        if (w->xmax[k] >= 1e10 && w->xmin[k] > -1e10) ADD_AI(k, -1.0, -1, 0.0, -w->xmin[k]);
    /* ibx upper: variable boxes, then the two-sided flow rows -rate <= Bf*Va <= rate */
    for (int k = 0; k < nx; ++k)
        if (fabs(w->xmax[k] - w->xmin[k]) > eps && w->xmax[k] < 1e10 && w->xmin[k] > -1e10)
            ADD_AI(k, 1.0, -1, 0.0, w->xmax[k]);
    for (int l = 0; l < nl; ++l)
        if (w->br_on[l] && c->br_rate[l] != 0)
            ADD_AI(c->br_from[l], c->br_b[l], c->br_to[l], -c->br_b[l], c->br_rate[l] / base);
    /* ibx lower */
    for (int k = 0; k < nx; ++k)
        if (fabs(w->xmax[k] - w->xmin[k]) > eps && w->xmax[k] < 1e10 && w->xmin[k] > -1e10)
            ADD_AI(k, -1.0, -1, 0.0, -w->xmin[k]);
    for (int l = 0; l < nl; ++l)
        if (w->br_on[l] && c->br_rate[l] != 0)
            ADD_AI(c->br_from[l], -c->br_b[l], c->br_to[l], c->br_b[l], c->br_rate[l] / base);
#undef ADD_AI

    /* ---- initialise (mips.m) ------------------------------------------------------- */
    double* x = w->x;
    double f = 0;
    for (int k = 0; k < nx; ++k) { x[k] = w->x0[k]; f += w->c[k] * x[k]; }
#define EVAL_H()                                                                          \
    for (int r = 0; r < niq; ++r) {                                                       \
        double s = w->ai_val[r * 2] * x[w->ai_idx[r * 2]];                               \
        if (w->ai_n[r] == 2) s += w->ai_val[r * 2 + 1] * x[w->ai_idx[r * 2 + 1]];         \
        w->h[r] = s - w->bi[r];                                                           \
    }
#define EVAL_G()                                                                          \
    for (int r = 0; r < neq; ++r) {                                                       \
        double s = 0;                                                                     \
        for (int e = 0; e < w->ae_n[r]; ++e) s += w->ae_val[r * w->rw + e] * x[w->ae_idx[r * w->rw + e]]; \
        w->g[r] = s - w->be[r];                                                           \
    }
#define EVAL_LX()                                                                         \
    for (int k = 0; k < nx; ++k) w->Lx[k] = w->c[k];                                      \
    for (int r = 0; r < neq; ++r)                                                         \
        for (int e = 0; e < w->ae_n[r]; ++e) w->Lx[w->ae_idx[r * w->rw + e]] += w->ae_val[r * w->rw + e] * w->lam[r]; \
    for (int r = 0; r < niq; ++r)                                                         \
        for (int e = 0; e < w->ai_n[r]; ++e) w->Lx[w->ai_idx[r * 2 + e]] += w->ai_val[r * 2 + e] * w->mu[r];
    EVAL_H(); EVAL_G();
    double gamma = 1.0;
    for (int r = 0; r < neq; ++r) w->lam[r] = 0.0;
    for (int r = 0; r < niq; ++r) {
        w->z[r] = o->z0; w->mu[r] = o->z0;
        if (w->h[r] < -o->z0) w->z[r] = -w->h[r];
        if (gamma / w->z[r] > o->z0) w->mu[r] = gamma / w->z[r];
    }
    double f0 = f;
    EVAL_LX();
    int converged = 0, eflag = 0, it = 0;
    /* (the pre-loop convergence test of mips.m can never pass: compcond = niq/(1+|x|) >> tol) */
    const int nk = nx + neq;
    while (!converged && it < o->max_it) {
        it++;
        /* M = Ai' diag(mu./z) Ai ; N = Lx + Ai' ((mu.*h + gamma)./z) */
        for (int i = 0; i < nk * nk; ++i) w->K[i] = 0.0;
        for (int k = 0; k < nx; ++k) w->N[k] = w->Lx[k];
        for (int r = 0; r < niq; ++r) {
            double zinv = 1.0 / w->z[r];
            double d = w->mu[r] * zinv;
            double t = (w->mu[r] * w->h[r] + gamma) * zinv;
            for (int a = 0; a < w->ai_n[r]; ++a) {
                int ia = w->ai_idx[r * 2 + a]; double va = w->ai_val[r * 2 + a];
                w->N[ia] += va * t;
                for (int b = 0; b < w->ai_n[r]; ++b)
                    w->K[ia * nk + w->ai_idx[r * 2 + b]] += va * d * w->ai_val[r * 2 + b];
            }
        }
        for (int r = 0; r < neq; ++r)
            for (int e = 0; e < w->ae_n[r]; ++e) {
                int k = w->ae_idx[r * w->rw + e]; double v = w->ae_val[r * w->rw + e];
                w->K[k * nk + nx + r] += v; w->K[(nx + r) * nk + k] += v;   /* parallel lines repeat (row, col) */
            }
        for (int k = 0; k < nx; ++k) w->rhs[k] = -w->N[k];
        for (int r = 0; r < neq; ++r) w->rhs[nx + r] = -w->g[r];
        int sing = lu_solve(w->K, nk, nk, w->rhs, w->piv);
        double nrm = 0; int bad = sing;
        for (int k = 0; k < nk && !bad; ++k) { if (w->rhs[k] != w->rhs[k]) bad = 1; nrm += w->rhs[k] * w->rhs[k]; }
        if (bad || sqrt(nrm) > o->max_stepsize) { eflag = -1; break; }
        const double* dx = w->rhs; const double* dlam = w->rhs + nx;
        double alphap = 1.0, alphad = 1.0, minp = INFINITY, mind = INFINITY;
        for (int r = 0; r < niq; ++r) {
            double s = w->ai_val[r * 2] * dx[w->ai_idx[r * 2]];
            if (w->ai_n[r] == 2) s += w->ai_val[r * 2 + 1] * dx[w->ai_idx[r * 2 + 1]];
            w->dz[r] = -w->h[r] - w->z[r] - s;
            w->dmu[r] = -w->mu[r] + (gamma - w->mu[r] * w->dz[r]) / w->z[r];
            if (w->dz[r] < 0) { double q = w->z[r] / -w->dz[r]; if (q < minp) minp = q; }
            if (w->dmu[r] < 0) { double q = w->mu[r] / -w->dmu[r]; if (q < mind) mind = q; }
        }
        if (minp < INFINITY) { alphap = o->xi * minp; if (alphap > 1.0) alphap = 1.0; }
        if (mind < INFINITY) { alphad = o->xi * mind; if (alphad > 1.0) alphad = 1.0; }
        for (int k = 0; k < nx; ++k) x[k] += alphap * dx[k];
        double zmu = 0;
        for (int r = 0; r < niq; ++r) { w->z[r] += alphap * w->dz[r]; w->mu[r] += alphad * w->dmu[r]; zmu += w->z[r] * w->mu[r]; }
        for (int r = 0; r < neq; ++r) w->lam[r] += alphad * dlam[r];
        if (niq > 0) gamma = o->sigma * zmu / niq;
        f = 0; for (int k = 0; k < nx; ++k) f += w->c[k] * x[k];
        EVAL_H(); EVAL_G(); EVAL_LX();
        double gmax = 0, hmax = -INFINITY, xmaxn = 0, zmaxn = 0, lxmax = 0, lammax = 0, mumax = 0;
        int xnan = 0;
        for (int r = 0; r < neq; ++r) { if (fabs(w->g[r]) > gmax) gmax = fabs(w->g[r]); if (fabs(w->lam[r]) > lammax) lammax = fabs(w->lam[r]); }
        for (int r = 0; r < niq; ++r) { if (w->h[r] > hmax) hmax = w->h[r]; if (fabs(w->z[r]) > zmaxn) zmaxn = fabs(w->z[r]); if (fabs(w->mu[r]) > mumax) mumax = fabs(w->mu[r]); }
        for (int k = 0; k < nx; ++k) { if (fabs(x[k]) > xmaxn) xmaxn = fabs(x[k]); if (fabs(w->Lx[k]) > lxmax) lxmax = fabs(w->Lx[k]); if (x[k] != x[k]) xnan = 1; }
        double feascond = (gmax > hmax ? gmax : hmax) / (1 + (xmaxn > zmaxn ? xmaxn : zmaxn));
        double gradcond = lxmax / (1 + (lammax > mumax ? lammax : mumax));
        double compcond = zmu / (1 + xmaxn);
        double costcond = fabs(f - f0) / (1 + fabs(f0));
        if (feascond < o->feastol && gradcond < o->gradtol && compcond < o->comptol && costcond < o->costtol) {
            converged = 1;
        } else {
            if (xnan || alphap < o->alpha_min || alphad < o->alpha_min || gamma < eps || gamma > 1 / eps) { eflag = -1; break; }
            f0 = f;
        }
    }
#undef EVAL_H
#undef EVAL_G
#undef EVAL_LX
    finish(c, w, ncol, f, scale, dns, nodal);
    *status = converged ? RELMC_ST_CONVERGED : (eflag == -1 ? RELMC_ST_NUMFAIL : RELMC_ST_MAXIT);
    *iters = it;
}

/* ------------------------------------------------------------------------------------ */
/* public oracle entry points                                                            */
/* ------------------------------------------------------------------------------------ */
int32_t orc_seq_mcsimulation(const relmc_case_desc* c, const uint8_t* states, const double* load_scale, int64_t n,
                             const relmc_solver_opts* opts, double* dns, double* nodal,
                             int32_t* status, int32_t* iters, int32_t* relaxed, int32_t nthreads)
{
    int ncomp = c->ng + c->nl;
    if (c->nb > RELMC_MAX_BUS || ncomp > RELMC_MAX_COMP) return RELMC_ERR_UNSUPPORTED;
    if (nthreads < 1) nthreads = 1;
#pragma omp parallel num_threads(nthreads)
    {
        orc_ws* w = ws_new(c);
        double nd[RELMC_MAX_BUS];
#pragma omp for schedule(dynamic, 16)
        for (int64_t i = 0; i < n; ++i) {
            double d; int32_t s, it, rx;
            solve_state(c, states + i * ncomp, load_scale ? load_scale[i] : 1.0, opts, w, &d, nd, &s, &it, &rx);
            dns[i] = d;
            if (nodal) memcpy(nodal + i * c->nb, nd, sizeof(double) * c->nb);
            if (status) status[i] = s;
            if (iters) iters[i] = it;
            if (relaxed) relaxed[i] = rx;
        }
        ws_free(w);
    }
    return RELMC_OK;
}

int32_t orc_mc_simulation(const relmc_case_desc* c, const uint8_t* states, int64_t n,
                          const relmc_solver_opts* opts, double* dns, double* nodal,
                          int32_t* status, int32_t* iters, int32_t* relaxed, int32_t nthreads)
{
    return orc_seq_mcsimulation(c, states, NULL, n, opts, dns, nodal, status, iters, relaxed, nthreads);
}

/* seq_mcsampling.m:35-76 for independent years (seqMain.m:91 calls it with num_years = 1, every year starts
 * all-up): TTF = round(-MTTF ln U), TTR = ceil(-MTTR ln U); U of event e of component k in global year y =
 * (philox(ctr=(y_lo, y_hi, k | 0x80000000, e >> 2), key = seed)[e & 3] + 0.5) / 2^32.
 * out[num_years][hpy][ncomp], 1 = down. */
int32_t orc_seq_mcsampling(int32_t ncomp, const double* mttf, const double* mttr, int32_t hpy, uint64_t seed,
                           uint64_t first_year, int32_t num_years, uint8_t* out)
{
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    memset(out, 0, (size_t)num_years * hpy * ncomp);
    for (int y = 0; y < num_years; ++y) {
        uint64_t gy = first_year + (uint64_t)y;
        for (int k = 0; k < ncomp; ++k) {
            long long current = 0; int up = 1; uint32_t r[4];
            for (int ev = 0; current < hpy; ++ev) {
                if ((ev & 3) == 0) {
                    uint32_t ctr[4] = {(uint32_t)gy, (uint32_t)(gy >> 32), (uint32_t)k | 0x80000000u, (uint32_t)(ev >> 2)};
                    philox4x32_10(ctr, key, r);
                }
                double u = ((double)r[ev & 3] + 0.5) * 2.3283064365386963e-10;
                if (up) {
                    current += (long long)floor(-mttf[k] * log(u) + 0.5);           /* round(), :53 */
                } else {
                    long long dur = (long long)ceil(-mttr[k] * log(u));             /* ceil(), :60 */
                    long long end = current + dur - 1;
                    if (end > hpy - 1) end = hpy - 1;
                    for (long long h = current; h <= end; ++h) out[((size_t)y * hpy + (size_t)h) * ncomp + k] = 1;   /* :63-68 */
                    current += dur;
                }
                up = !up;
            }
        }
    }
    return RELMC_OK;
}

/* seqMain.m:85-176 for years [first_year, first_year + n_years): years_out[y] = {ens, dlc, nlc, n_contingency};
 * acc: n = LPs, n_fail = loss hours, comp_fail = component-down counts during loss, sum_nodal = nodal MWh */
int32_t orc_seq_years(const relmc_case_desc* c, const double* mttf, const double* mttr, int32_t hpy, const double* load_factors,
                      uint64_t seed, uint64_t first_year, int32_t n_years, const relmc_solver_opts* opts, double threshold,
                      int32_t nthreads, double* years_out, relmc_acc* acc)
{
    int ncomp = c->ng + c->nl;
    if (nthreads < 1) nthreads = 1;
    memset(acc, 0, sizeof(*acc));
    uint8_t* states = (uint8_t*)xm((size_t)hpy * ncomp);
    double* curt = (double*)xm(sizeof(double) * hpy);
    double* nod = (double*)xm(sizeof(double) * (size_t)hpy * c->nb);
    int32_t* stat = (int32_t*)xm(sizeof(int32_t) * hpy); int32_t* its = (int32_t*)xm(sizeof(int32_t) * hpy); int32_t* rlx = (int32_t*)xm(sizeof(int32_t) * hpy);
    int* hours = (int*)xm(sizeof(int) * hpy);
    uint8_t* cst = (uint8_t*)xm((size_t)hpy * ncomp);
    double* csc = (double*)xm(sizeof(double) * hpy);
    for (int y = 0; y < n_years; ++y) {
        orc_seq_mcsampling(ncomp, mttf, mttr, hpy, seed, first_year + (uint64_t)y, 1, states);
        int nc = 0;
        for (int h = 0; h < hpy; ++h) {                                    /* contingency hours, :97 */
            int any = 0;
            for (int k = 0; k < ncomp; ++k) any |= states[(size_t)h * ncomp + k];
            if (any) { memcpy(cst + (size_t)nc * ncomp, states + (size_t)h * ncomp, ncomp); csc[nc] = load_factors[h]; hours[nc++] = h; }
        }
        orc_seq_mcsimulation(c, cst, csc, nc, opts, curt, nod, stat, its, rlx, nthreads);   /* :112-133 */
        double* prof = (double*)xm(sizeof(double) * hpy);
        double ens = 0, dlc = 0, nlc = 0;
        for (int j = 0; j < nc; ++j) {
            prof[hours[j]] = curt[j];
            acc->n += 1; acc->sum_iters += its[j]; acc->sum_dns += curt[j]; acc->sum_dns2 += curt[j] * curt[j];
            if (stat[j] == RELMC_ST_SINGULAR) acc->n_singular += 1;
            if (stat[j] == RELMC_ST_MAXIT || stat[j] == RELMC_ST_NUMFAIL) acc->n_nonconverged += 1;
            if (rlx[j]) acc->n_infeasible += 1;
            if (curt[j] > threshold) {                                      /* loss hour, :144-158 */
                acc->n_fail += 1;
                for (int i = 0; i < c->nb; ++i) acc->sum_nodal[i] += nod[(size_t)j * c->nb + i];
                for (int k = 0; k < ncomp; ++k) acc->comp_fail[k] += cst[(size_t)j * ncomp + k];
            }
        }
        for (int h = 0; h < hpy; ++h) {                                    /* :136-176, calnlc.m:22-32 */
            int f = prof[h] > threshold;
            ens += prof[h];
            if (f) { dlc += 1; if (h == 0 || !(prof[h - 1] > threshold)) nlc += 1; }
        }
        free(prof);
        years_out[4 * y] = ens; years_out[4 * y + 1] = dlc; years_out[4 * y + 2] = nlc; years_out[4 * y + 3] = nc;
    }
    free(states); free(curt); free(nod); free(stat); free(its); free(rlx); free(hours); free(cst); free(csc);
    return RELMC_OK;
}

/* memo cache (test speed-up only; the reference's own state_database, nsqMain.m:220-245) */
typedef struct { uint64_t k[4]; double dns; int32_t status, iters, relaxed; int used; double nodal[RELMC_MAX_BUS]; } memo_ent;
typedef struct { memo_ent* e; size_t cap, n; } memo_t;

static uint64_t mix64(uint64_t x) { x ^= x >> 33; x *= 0xff51afd7ed558ccdULL; x ^= x >> 33; x *= 0xc4ceb9fe1a85ec53ULL; x ^= x >> 33; return x; }

static memo_ent* memo_find(memo_t* m, const uint64_t k[4])
{
    if (m->n * 2 >= m->cap) {
        size_t ncap = m->cap ? m->cap * 2 : 1024;
        memo_ent* ne = (memo_ent*)xm(sizeof(memo_ent) * ncap);
        for (size_t i = 0; i < m->cap; ++i) if (m->e[i].used) {
            size_t p = mix64(m->e[i].k[0] ^ mix64(m->e[i].k[1] ^ mix64(m->e[i].k[2] ^ mix64(m->e[i].k[3])))) & (ncap - 1);
            while (ne[p].used) p = (p + 1) & (ncap - 1);
            ne[p] = m->e[i];
        }
        free(m->e); m->e = ne; m->cap = ncap;
    }
    size_t p = mix64(k[0] ^ mix64(k[1] ^ mix64(k[2] ^ mix64(k[3])))) & (m->cap - 1);
    while (m->e[p].used) {
        if (m->e[p].k[0] == k[0] && m->e[p].k[1] == k[1] && m->e[p].k[2] == k[2] && m->e[p].k[3] == k[3]) return &m->e[p];
        p = (p + 1) & (m->cap - 1);
    }
    memcpy(m->e[p].k, k, sizeof(uint64_t) * 4);
    return &m->e[p];
}

static void acc_add(relmc_acc* a, const relmc_case_desc* c, const uint8_t* st, double dns,
                    const double* nodal, int32_t status, int32_t iters, int32_t relaxed)
{
    int ncomp = c->ng + c->nl;
    a->n += 1;
    a->sum_dns += dns;
    a->sum_dns2 += dns * dns;
    a->sum_iters += iters;
    if (status == RELMC_ST_SINGULAR) a->n_singular += 1;
    if (status == RELMC_ST_MAXIT || status == RELMC_ST_NUMFAIL) a->n_nonconverged += 1;
    if (relaxed) a->n_infeasible += 1;
    for (int i = 0; i < c->nb; ++i) a->sum_nodal[i] += nodal[i];
    if (dns > 1e-4) {                                    /* nsqMain.m:270 */
        a->n_fail += 1;
        for (int k = 0; k < ncomp; ++k) a->comp_fail[k] += st[k];
    }
}

static void acc_merge(relmc_acc* d, const relmc_acc* s)
{
    d->n += s->n; d->n_fail += s->n_fail; d->n_singular += s->n_singular;
    d->n_infeasible += s->n_infeasible; d->n_nonconverged += s->n_nonconverged;
    d->sum_iters += s->sum_iters; d->sum_dns += s->sum_dns; d->sum_dns2 += s->sum_dns2;
    for (int k = 0; k < RELMC_MAX_COMP; ++k) d->comp_fail[k] += s->comp_fail[k];
    for (int i = 0; i < RELMC_MAX_BUS; ++i) d->sum_nodal[i] += s->sum_nodal[i];
}

int32_t orc_nsq_accumulate(const relmc_case_desc* c, uint64_t seed, uint64_t first_index, int64_t n,
                           const relmc_solver_opts* opts, int32_t nthreads, int32_t use_memo,
                           relmc_acc* acc_out)
{
    int ncomp = c->ng + c->nl;
    if (c->nb > RELMC_MAX_BUS || ncomp > RELMC_MAX_COMP) return RELMC_ERR_UNSUPPORTED;
    if (nthreads < 1) nthreads = 1;
    uint32_t thr[RELMC_MAX_COMP];
    orc_thresholds(c, thr);
    relmc_acc* part = (relmc_acc*)xm(sizeof(relmc_acc) * nthreads);
#pragma omp parallel num_threads(nthreads)
    {
#ifdef _OPENMP
        int tid = omp_get_thread_num();
#else
        int tid = 0;
#endif
        orc_ws* w = ws_new(c);
        memo_t memo = {0, 0, 0};
        uint8_t st[RELMC_MAX_COMP];
        double nd[RELMC_MAX_BUS];
        /* contiguous chunk per thread, merged in thread order: deterministic sums */
        int64_t lo = n * tid / nthreads, hi = n * (tid + 1) / nthreads;
        for (int64_t i = lo; i < hi; ++i) {
            double d; int32_t s, it, rx;
            sample_state(thr, ncomp, seed, first_index + (uint64_t)i, st);
            if (use_memo && ncomp <= 256) {
                uint64_t key[4] = {0, 0, 0, 0};
                for (int k = 0; k < ncomp; ++k) if (st[k]) key[k >> 6] |= 1ULL << (k & 63);
                memo_ent* e = memo_find(&memo, key);
                if (!e->used) {
                    solve_state(c, st, 1.0, opts, w, &e->dns, e->nodal, &e->status, &e->iters, &e->relaxed);
                    e->used = 1; memo.n++;
                }
                acc_add(&part[tid], c, st, e->dns, e->nodal, e->status, e->iters, e->relaxed);
            } else {
                solve_state(c, st, 1.0, opts, w, &d, nd, &s, &it, &rx);
                acc_add(&part[tid], c, st, d, nd, s, it, rx);
            }
        }
        free(memo.e);
        ws_free(w);
    }
    memset(acc_out, 0, sizeof(*acc_out));
    for (int t = 0; t < nthreads; ++t) acc_merge(acc_out, &part[t]);
    free(part);
    return RELMC_OK;
}

/* ---- nsqMain.m:208-308 restated literally in DATABASE form (the checker of the device state database) -----------
 * Per batch: mc_sampling (:212); unique(rows,'stable') with counts (:220-229); intersect with the database -> bump the
 * counts of known states, drop them (:232-245); evaluate the new states (parfor, :257-263); append [state, count, dns,
 * flag, nodal] (:269-278); indices from ALL rows (:282-301, beta with the central sum as written there); histories
 * (:304-308).  Loop condition of :208.  Rows come out in the order the reference would hold them. */
typedef struct { uint64_t k[4]; int64_t row; int used; } dbmap_ent;
typedef struct { dbmap_ent* e; size_t cap, n; } dbmap_t;
static dbmap_ent* dbmap_find(dbmap_t* m, const uint64_t k[4])
{
    if (m->n * 2 >= m->cap) {
        size_t ncap = m->cap ? m->cap * 2 : 1024;
        dbmap_ent* ne = (dbmap_ent*)xm(sizeof(dbmap_ent) * ncap);
        for (size_t i = 0; i < m->cap; ++i) if (m->e[i].used) {
            size_t p = mix64(m->e[i].k[0] ^ mix64(m->e[i].k[1] ^ mix64(m->e[i].k[2] ^ mix64(m->e[i].k[3])))) & (ncap - 1);
            while (ne[p].used) p = (p + 1) & (ncap - 1);
            ne[p] = m->e[i];
        }
        free(m->e); m->e = ne; m->cap = ncap;
    }
    size_t p = mix64(k[0] ^ mix64(k[1] ^ mix64(k[2] ^ mix64(k[3])))) & (m->cap - 1);
    while (m->e[p].used) {
        if (m->e[p].k[0] == k[0] && m->e[p].k[1] == k[1] && m->e[p].k[2] == k[2] && m->e[p].k[3] == k[3]) return &m->e[p];
        p = (p + 1) & (m->cap - 1);
    }
    memcpy(m->e[p].k, k, sizeof(uint64_t) * 4);
    return &m->e[p];
}

int32_t orc_nsq_database(const relmc_case_desc* c, uint64_t seed, double beta_limit, int64_t max_iterations, int64_t samples_per_batch,
                         const relmc_solver_opts* opts, int32_t nthreads, int64_t max_rows,
                         uint8_t* db_states, int64_t* db_count, double* db_dns, int32_t* db_flag, double* db_nodal,
                         int32_t* db_status, int32_t* db_iters, int32_t* db_relaxed, int64_t* rows_out,
                         int64_t hist_cap, double* beta_hist, double* edns_hist, double* lole_hist, double* plc_hist,
                         int64_t* checkpoints_out, int64_t* iterations_out, relmc_acc* acc_out)
{
    const int ncomp = c->ng + c->nl, nb = c->nb;
    if (nb > RELMC_MAX_BUS || ncomp > RELMC_MAX_COMP || samples_per_batch < 1) return RELMC_ERR_UNSUPPORTED;
    if (nthreads < 1) nthreads = 1;
    uint32_t thr[RELMC_MAX_COMP];
    orc_thresholds(c, thr);
    dbmap_t dbm = {0, 0, 0};
    int64_t rows = 0, current_iteration = 0, cp = 0;
    double current_beta = INFINITY;
    uint8_t* bst = (uint8_t*)xm((size_t)samples_per_batch * ncomp);          /* the batch's unique states, in order of appearance */
    int64_t* bcnt = (int64_t*)xm(sizeof(int64_t) * samples_per_batch);
    int64_t* newrow = (int64_t*)xm(sizeof(int64_t) * samples_per_batch);
    orc_ws** ws = (orc_ws**)xm(sizeof(orc_ws*) * nthreads);
    for (int t = 0; t < nthreads; ++t) ws[t] = ws_new(c);
    int32_t rc = RELMC_OK;
    while (current_beta > beta_limit && current_iteration < max_iterations) {          /* nsqMain.m:208 */
        /* :212 + :220-229: sample, unique rows in order of first appearance, counts */
        dbmap_t bm = {0, 0, 0};
        int64_t nuniq = 0;
        uint8_t st[RELMC_MAX_COMP];
        for (int64_t i = 0; i < samples_per_batch; ++i) {
            sample_state(thr, ncomp, seed, (uint64_t)(current_iteration + i), st);
            uint64_t key[4] = {0, 0, 0, 0};
            for (int k = 0; k < ncomp; ++k) if (st[k]) key[k >> 6] |= 1ULL << (k & 63);
            dbmap_ent* e = dbmap_find(&bm, key);
            if (!e->used) { e->used = 1; bm.n++; e->row = nuniq; memcpy(bst + (size_t)nuniq * ncomp, st, (size_t)ncomp); bcnt[nuniq] = 0; nuniq++; }
            bcnt[e->row] += 1;
        }
        free(bm.e);
        /* :232-245: states already in the database collect the batch's counts; the others are new */
        int64_t nnew = 0;
        for (int64_t u = 0; u < nuniq; ++u) {
            const uint8_t* s_ = bst + (size_t)u * ncomp;
            uint64_t key[4] = {0, 0, 0, 0};
            for (int k = 0; k < ncomp; ++k) if (s_[k]) key[k >> 6] |= 1ULL << (k & 63);
            dbmap_ent* e = dbmap_find(&dbm, key);
            if (e->used) db_count[e->row] += bcnt[u];
            else {
                if (rows + nnew >= max_rows) { rc = RELMC_ERR_UNSUPPORTED; goto done; }
                e->used = 1; dbm.n++; e->row = rows + nnew;
                memcpy(db_states + (size_t)e->row * ncomp, s_, (size_t)ncomp);
                db_count[e->row] = bcnt[u];
                newrow[nnew++] = e->row;
            }
        }
        /* :257-263 (parfor) + :269-278 */
#pragma omp parallel for num_threads(nthreads) schedule(dynamic, 4)
        for (int64_t q = 0; q < nnew; ++q) {
#ifdef _OPENMP
            orc_ws* w = ws[omp_get_thread_num()];
#else
            orc_ws* w = ws[0];
#endif
            const int64_t r = newrow[q];
            solve_state(c, db_states + (size_t)r * ncomp, 1.0, opts, w, &db_dns[r], db_nodal + (size_t)r * nb, &db_status[r], &db_iters[r], &db_relaxed[r]);
            db_flag[r] = db_dns[r] > 1e-4 ? 1 : 0;                                       /* :270 */
        }
        rows += nnew;
        /* :282-301 */
        const double current_samples = (double)(current_iteration + samples_per_batch);
        double sdns = 0.0, sflag = 0.0;
        for (int64_t r = 0; r < rows; ++r) { sdns += (double)db_count[r] * db_dns[r]; sflag += (double)db_count[r] * (double)db_flag[r]; }
        const double edns = sdns / current_samples;
        const double lole = sflag / current_samples * 8760.0;
        const double plc = sflag / current_samples;
        double ss = 0.0;
        for (int64_t r = 0; r < rows; ++r) { const double d = db_dns[r] - edns; ss += (double)db_count[r] * d * d; }
        current_beta = sqrt(ss) / current_samples / edns;
        if (cp < hist_cap) { beta_hist[cp] = current_beta; edns_hist[cp] = edns; lole_hist[cp] = lole; plc_hist[cp] = plc; }   /* :304-308 */
        cp++;
        current_iteration += samples_per_batch;
    }
done:
    /* the additive accumulators of include/relmc.h from the database rows (what the device path all-reduces) */
    if (acc_out) {
        memset(acc_out, 0, sizeof(*acc_out));
        for (int64_t r = 0; r < rows; ++r) {
            const int64_t cn = db_count[r];
            acc_out->n += cn;
            acc_out->sum_dns += (double)cn * db_dns[r];
            acc_out->sum_dns2 += (double)cn * db_dns[r] * db_dns[r];
            acc_out->sum_iters += cn * db_iters[r];
            if (db_status[r] == RELMC_ST_SINGULAR) acc_out->n_singular += cn;
            if (db_status[r] == RELMC_ST_MAXIT || db_status[r] == RELMC_ST_NUMFAIL) acc_out->n_nonconverged += cn;
            if (db_relaxed[r]) acc_out->n_infeasible += cn;
            for (int i = 0; i < nb; ++i) acc_out->sum_nodal[i] += (double)cn * db_nodal[(size_t)r * nb + i];
            if (db_flag[r]) {
                acc_out->n_fail += cn;
                for (int k = 0; k < ncomp; ++k) acc_out->comp_fail[k] += cn * db_states[(size_t)r * ncomp + k];
            }
        }
    }
    *rows_out = rows; *checkpoints_out = cp; *iterations_out = current_iteration;
    for (int t = 0; t < nthreads; ++t) ws_free(ws[t]);
    free(ws); free(bst); free(bcnt); free(newrow); free(dbm.e);
    return rc;
}

/* estimators, nsqMain.m:282-301, 348-349, 366-376 (independent restatement of relmc_nsq_indices) */
void orc_nsq_indices(const relmc_acc* a, int32_t nb, int32_t ncomp, double hours, relmc_indices* out)
{
    memset(out, 0, sizeof(*out));
    out->n = a->n;
    if (a->n <= 0) return;
    double N = (double)a->n;
    out->edns = a->sum_dns / N;
    out->plc = (double)a->n_fail / N;
    out->lole = out->plc * hours;
    out->eens = out->edns * hours;
    double ss = a->sum_dns2 - N * out->edns * out->edns;     /* sum (dns - EDNS)^2 */
    if (ss < 0) ss = 0;
    out->beta = out->edns > 0 ? sqrt(ss) / N / out->edns : INFINITY;
    out->mean_iters = (double)a->sum_iters / N;
    for (int i = 0; i < nb; ++i) out->nodal_eens[i] = a->sum_nodal[i] / N;
    for (int k = 0; k < ncomp; ++k) out->comp_importance[k] = a->n_fail ? (double)a->comp_fail[k] / (double)a->n_fail : 0.0;
}

/* HL1 copper sheet — GeneratingAdequacy/PowerSystemAdequacy.jl:169-208 run_non_sequential_mc, restated:
 * per iteration sample every unit (up iff rand() >= for_rate, :183-185; here: down iff draw_u32 < floor(FOR*2^32)
 * of the same counter-based stream), then sweep ALL hourly loads (:191-197). */
int32_t orc_hl1_nsq(int32_t ngen, const double* cap, const double* for_rate, int32_t nhours, const double* load,
                    uint64_t seed, uint64_t first_index, int64_t n, double* iter_lole, double* iter_eue)
{
    uint32_t key[2] = {(uint32_t)seed, (uint32_t)(seed >> 32)};
    for (int64_t i = 0; i < n; ++i) {
        uint64_t gi = first_index + (uint64_t)i;
        double cap_avail = 0.0;
        for (int blk = 0; blk * 4 < ngen; ++blk) {
            uint32_t ctr[4] = {(uint32_t)gi, (uint32_t)(gi >> 32), (uint32_t)blk, 0u}, r[4];
            philox4x32_10(ctr, key, r);
            for (int e = 0; e < 4 && blk * 4 + e < ngen; ++e) {
                double t = floor(for_rate[blk * 4 + e] * 4294967296.0);   /* clamped to [0, 2^32 - 1] as relmc_hl1_load (include/relmc.h) */
                if (!(t > 0)) t = 0;
                if (t > 4294967295.0) t = 4294967295.0;
                if (!(r[e] < (uint32_t)t)) cap_avail += cap[blk * 4 + e];
            }
        }
        double lole = 0.0, eue = 0.0;
        for (int h = 0; h < nhours; ++h)
            if (cap_avail < load[h]) { lole += 1.0; eue += load[h] - cap_avail; }
        iter_lole[i] = lole; iter_eue[i] = eue;
    }
    return RELMC_OK;
}

int32_t orc_max_threads(void)
{
#ifdef _OPENMP
    return omp_get_max_threads();
#else
    return 1;
#endif
}
