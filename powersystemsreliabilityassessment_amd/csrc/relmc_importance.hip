// relmc_importance.hip — importance sampling for the non-sequential HL2 Monte Carlo (contract in include/relmc.h): the tilt's thresholds and
// likelihood-ratio tables (host), the tilted sampler and the weighted reductions (kernels in relmc_is_kernels.h), the weighted estimators,
// the cross-entropy tuner and the weighted run loop.  States are evaluated by the existing relmc_mc_simulation_dev path, retry ladder included.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"      // hl1_reduce_blocks: the weighted reductions take the HL1 record reduction's grid rule
#include "relmc_is_kernels.h"

namespace relmc_host {

namespace {

constexpr int64_t kIsLaunch = (int64_t)1 << 20;       // samples per launch: bounds the per-sample buffers (states, W, dns, nodal, status, iters, factors)
constexpr int64_t kIsColChunk = 1024;                 // samples per workgroup of the column sums
constexpr double kTwo32 = 4294967296.0;

// why a tilt is refused: 1 = entry not finite or outside [0, 1], 2 = thr_is == 0 where thr > 0
int is_ratios_impl(int ncomp, const uint32_t* thr, const uint8_t* always_up, const double* unavail_is, uint32_t* thr_is, double* r_dn, double* r_up,
                   int* bad, int* why)
{
    *bad = -1; *why = 0;
    std::vector<uint32_t> t((size_t)ncomp);
    for (int k = 0; k < ncomp; ++k) {
        if (!unavail_is) { t[k] = thr[k]; continue; }
        const double u = unavail_is[k];
        if (!(std::isfinite(u) && u >= 0.0 && u <= 1.0)) { *bad = k; *why = 1; return RELMC_ERR_INVALID; }
        double f = std::floor(u * kTwo32);                          // relmc_case_load's rule (relmc_schedule.hip)
        if (!(f > 0)) f = 0;
        if (f > 4294967295.0) f = 4294967295.0;
        t[k] = always_up && always_up[k] ? 0u : (uint32_t)f;
        if (t[k] == 0 && thr[k] > 0) { *bad = k; *why = 2; return RELMC_ERR_INVALID; }
    }
    for (int k = 0; k < ncomp; ++k) {                               // nothing is written before the whole tilt has passed
        if (thr_is) thr_is[k] = t[k];
        if (r_dn) r_dn[k] = t[k] ? (double)thr[k] / (double)t[k] : 1.0;
        if (r_up) r_up[k] = (kTwo32 - (double)thr[k]) / (kTwo32 - (double)t[k]);
    }
    return RELMC_OK;
}

const uint32_t* case_thr(const relmc_ctx* ctx) { return ctx->tile == 0 ? ctx->hcase24.thr : ctx->hcase96.thr; }

// validates the tilt against the loaded case and puts its three tables into the context's device buffers
int tilt_upload(relmc_ctx* ctx, const char* who, const double* unavail_is)
{
    const int nc = ctx->ncomp;
    std::vector<uint32_t> t((size_t)nc); std::vector<double> dn((size_t)nc), up((size_t)nc);
    int bad = -1, why = 0;
    const uint8_t* au = ctx->case_copy.valid ? ctx->case_copy.always_up.data() : nullptr;
    if (is_ratios_impl(nc, case_thr(ctx), au, unavail_is, t.data(), dn.data(), up.data(), &bad, &why))
        return fail(ctx, RELMC_ERR_INVALID, std::string(who) + ": unavail_is of component " + std::to_string(bad) +
                                                (why == 1 ? " is not a number in [0, 1]" : " is zero although the case's own is not: the tilted law must cover the nominal one"));
    auto& S = ctx->is;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, S.thr.grow(RELMC_MAX_COMP)); HIP_TRY(ctx, S.r_dn.grow(RELMC_MAX_COMP)); HIP_TRY(ctx, S.r_up.grow(RELMC_MAX_COMP));
    HIP_TRY(ctx, hipMemcpyAsync(S.thr.get(), t.data(), sizeof(uint32_t) * nc, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(S.r_dn.get(), dn.data(), sizeof(double) * nc, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(S.r_up.get(), up.data(), sizeof(double) * nc, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));               // the host vectors end with this function
    return RELMC_OK;
}

// the sampler over [first_index, first_index + n) with the tables of the last tilt_upload, queued on the context's stream
int sample_queue(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, uint8_t* states_dev, double* w_dev)
{
    int64_t blocks = (n + IS_THREADS - 1) / IS_THREADS;
    if (blocks > (int64_t)ctx->num_cu * 8) blocks = (int64_t)ctx->num_cu * 8;
    const size_t lds = states_dev ? (size_t)IS_THREADS * ctx->ncomp : 0;
    hipLaunchKernelGGL(relmc_is_sampling_kernel, dim3((unsigned)blocks), dim3(IS_THREADS), lds, ctx->stream, ctx->is.thr.get(), ctx->is.r_dn.get(), ctx->is.r_up.get(),
                       ctx->ncomp, seed, first_index, n, states_dev, w_dev);
    HIP_TRY(ctx, hipGetLastError());
    return RELMC_OK;
}

// column sums of rows[n][ncols] under `factor` into sum[ncols] (+=), block partials added in block order; `part` = this call's slice of
// ctx->is.part_col (blocks * ncols doubles), copied back by the caller's synchronisation
template <class T>
int colsum_queue(relmc_ctx* ctx, const T* rows, int ncols, const double* factor, int64_t n, double* part)
{
    const int64_t blocks = (n + kIsColChunk - 1) / kIsColChunk;
    hipLaunchKernelGGL(relmc_is_colsum_kernel<T>, dim3((unsigned)blocks), dim3(IS_THREADS), 0, ctx->stream, rows, ncols, factor, n, kIsColChunk, part);
    HIP_TRY(ctx, hipGetLastError());
    return RELMC_OK;
}
void colsum_add(const double* part, int64_t blocks, int ncols, double* sum)
{
    for (int64_t b = 0; b < blocks; ++b)
        for (int t = 0; t < ncols; ++t) sum[t] += part[(size_t)b * ncols + t];
}

// a pair of events of one call (the context's own pair times the evaluation launches)
struct EventPair {
    hipEvent_t a = nullptr, b = nullptr;
    ~EventPair() { if (a) (void)hipEventDestroy(a); if (b) (void)hipEventDestroy(b); }
    hipError_t create() { const hipError_t e = hipEventCreate(&a); return e != hipSuccess ? e : hipEventCreate(&b); }
    float ms() const { float t = 0.f; return hipEventElapsedTime(&t, a, b) == hipSuccess ? t : 0.f; }
};

// per-sample buffers of a launch of m samples; nodal / status / iters / factors only for the accumulators
int buffers_ensure(relmc_ctx* ctx, int64_t m, bool full)
{
    auto& S = ctx->is;
    const size_t n = (size_t)m;
    HIP_TRY(ctx, S.states.grow(n * ctx->ncomp)); HIP_TRY(ctx, S.w.grow(n)); HIP_TRY(ctx, S.dns.grow(n));
    const size_t cb = (size_t)((m + kIsColChunk - 1) / kIsColChunk);
    HIP_TRY(ctx, S.part_col.grow(cb * (2 * (size_t)ctx->ncomp + ctx->nb)));
    if (!full) { HIP_TRY(ctx, S.e.grow(n)); return RELMC_OK; }
    HIP_TRY(ctx, S.nodal.grow(n * ctx->nb)); HIP_TRY(ctx, S.status.grow(n)); HIP_TRY(ctx, S.iters.grow(n));
    HIP_TRY(ctx, S.f_fail.grow(n)); HIP_TRY(ctx, S.f_dns.grow(n));
    const size_t sb = (size_t)hl1_reduce_blocks(m);
    HIP_TRY(ctx, S.part_d.grow(sb * 6)); HIP_TRY(ctx, S.part_i.grow(sb * 4));
    return RELMC_OK;
}

// one launch of the accumulators: m <= kIsLaunch samples, tables uploaded; adds to *out and to *ms
int accumulate_launch(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t m, const relmc_solver_opts& o, relmc_is_acc* out, double* ms)
{
    auto& S = ctx->is;
    const int nc = ctx->ncomp, nb = ctx->nb;
    int rc = buffers_ensure(ctx, m, true);
    if (rc) return rc;
    EventPair es, er;
    HIP_TRY(ctx, es.create()); HIP_TRY(ctx, er.create());
    HIP_TRY(ctx, hipEventRecord(es.a, ctx->stream));
    rc = sample_queue(ctx, seed, first_index, m, S.states.get(), S.w.get());
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(es.b, ctx->stream));
    int64_t n_infeasible = 0;
    rc = mc_simulation_dev_impl(ctx, S.states.get(), m, &o, S.dns.get(), S.nodal.get(), S.status.get(), S.iters.get(), &n_infeasible);
    if (rc) return rc;
    const double ms_eval = ctx->last_kernel_ms;
    const int64_t sb = hl1_reduce_blocks(m), cb = (m + kIsColChunk - 1) / kIsColChunk;
    double* const pc = S.part_col.get();
    HIP_TRY(ctx, hipEventRecord(er.a, ctx->stream));
    hipLaunchKernelGGL(relmc_is_scalar_kernel, dim3((unsigned)sb), dim3(IS_THREADS), 0, ctx->stream, m, S.w.get(), S.dns.get(), S.status.get(), S.iters.get(),
                       1e-4 /* nsqMain.m:270 */, S.f_fail.get(), S.f_dns.get(), S.part_d.get(), S.part_i.get());
    HIP_TRY(ctx, hipGetLastError());
    rc = colsum_queue<uint8_t>(ctx, S.states.get(), nc, S.f_fail.get(), m, pc);
    if (rc == RELMC_OK) rc = colsum_queue<uint8_t>(ctx, S.states.get(), nc, S.f_dns.get(), m, pc + (size_t)cb * nc);
    if (rc == RELMC_OK) rc = colsum_queue<double>(ctx, S.nodal.get(), nb, S.w.get(), m, pc + (size_t)cb * 2 * nc);
    if (rc) return rc;
    HIP_TRY(ctx, hipEventRecord(er.b, ctx->stream));
    std::vector<double> pd((size_t)sb * 6), col((size_t)cb * (2 * (size_t)nc + nb));
    std::vector<long long> pi((size_t)sb * 4);
    HIP_TRY(ctx, hipMemcpyAsync(pd.data(), S.part_d.get(), sizeof(double) * pd.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(pi.data(), S.part_i.get(), sizeof(long long) * pi.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipMemcpyAsync(col.data(), pc, sizeof(double) * col.size(), hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    *ms += (double)es.ms() + ms_eval + (double)er.ms();
    relmc_is_acc part;
    relmc_is_acc_zero(&part);
    part.n = m; part.n_infeasible = n_infeasible;
    for (int64_t b = 0; b < sb; ++b) {                              // block order: part of the results
        const double* d = &pd[(size_t)b * 6]; const long long* c = &pi[(size_t)b * 4];
        part.sum_w += d[0]; part.sum_w2 += d[1]; part.sum_wfail += d[2]; part.sum_w2fail += d[3]; part.sum_wdns += d[4]; part.sum_w2dns2 += d[5];
        part.n_fail += c[0]; part.n_singular += c[1]; part.n_nonconverged += c[2]; part.sum_iters += c[3];
    }
    colsum_add(col.data(), cb, nc, part.comp_wfail);
    colsum_add(col.data() + (size_t)cb * nc, cb, nc, part.comp_wdns);
    colsum_add(col.data() + (size_t)cb * 2 * nc, cb, nb, part.sum_wnodal);
    relmc_is_acc_merge(out, &part);
    return RELMC_OK;
}

int accumulate_impl(relmc_ctx* ctx, const char* who, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts, const double* unavail_is,
                    relmc_is_acc* out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, std::string(who) + ": no case loaded");
    if (n < 0 || !out) return fail(ctx, RELMC_ERR_INVALID, std::string(who) + ": bad arguments");
    int rc = tilt_upload(ctx, who, unavail_is);
    if (rc) return rc;
    relmc_is_acc_zero(out);
    if (n == 0) return RELMC_OK;
    relmc_solver_opts o = solver_opts_or_default(opts);
    o.screen = 0;                                                   // relmc_mc_simulation solves what it is handed
    double ms = 0.0;
    for (int64_t done = 0; done < n;) {
        const int64_t m = n - done < kIsLaunch ? n - done : kIsLaunch;
        rc = accumulate_launch(ctx, seed, first_index + (uint64_t)done, m, o, out, &ms);
        if (rc) return rc;
        done += m;
    }
    ctx->last_kernel_ms = ms;
    return RELMC_OK;
}

// relmc_nsq_indices' beta (nsqMain.m:299-301 with the guard of SURVEY.md App. E) from a sum and a sum of squares
double beta_of(double sum, double sum2, double N)
{
    const double mean = sum / N;
    double ss = sum2 - N * mean * mean;
    if (ss < 0) ss = 0;
    return mean > 0 ? std::sqrt(ss) / N / mean : INFINITY;
}

}  // namespace

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

int32_t relmc_is_ratios(int32_t ncomp, const uint32_t* thr, const uint8_t* always_up, const double* unavail_is, uint32_t* thr_is_out,
                        double* r_dn_out, double* r_up_out, int32_t* bad_component_out)
{
    if (bad_component_out) *bad_component_out = -1;
    if (ncomp < 0 || ncomp > RELMC_MAX_COMP || (ncomp > 0 && !thr)) return RELMC_ERR_INVALID;
    int bad = -1, why = 0;
    const int rc = is_ratios_impl(ncomp, thr, always_up, unavail_is, thr_is_out, r_dn_out, r_up_out, &bad, &why);
    if (bad_component_out) *bad_component_out = bad;
    return rc;
}

int32_t relmc_is_sampling_dev(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const double* unavail_is, uint8_t* eqstatus_dev,
                              double* weight_dev)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_is_sampling: no case loaded");
    if (n < 0) return fail(ctx, RELMC_ERR_INVALID, "relmc_is_sampling: bad arguments");
    int rc = tilt_upload(ctx, "relmc_is_sampling", unavail_is);
    if (rc || n == 0 || (!eqstatus_dev && !weight_dev)) return rc;
    rc = sample_queue(ctx, seed, first_index, n, eqstatus_dev, weight_dev);
    if (rc) return rc;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return RELMC_OK;
}

int32_t relmc_is_sampling(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const double* unavail_is, uint8_t* eqstatus_host,
                          double* weight_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_is_sampling: no case loaded");
    if (n < 0) return fail(ctx, RELMC_ERR_INVALID, "relmc_is_sampling: bad arguments");
    int rc = tilt_upload(ctx, "relmc_is_sampling", unavail_is);
    if (rc || n == 0 || (!eqstatus_host && !weight_host)) return rc;
    auto& S = ctx->is;
    const size_t nc = (size_t)ctx->ncomp;
    for (int64_t done = 0; done < n;) {                             // through the context's launch-sized buffers
        const int64_t m = n - done < kIsLaunch ? n - done : kIsLaunch;
        if (eqstatus_host) HIP_TRY(ctx, S.states.grow((size_t)m * nc));
        if (weight_host) HIP_TRY(ctx, S.w.grow((size_t)m));
        rc = sample_queue(ctx, seed, first_index + (uint64_t)done, m, eqstatus_host ? S.states.get() : nullptr, weight_host ? S.w.get() : nullptr);
        if (rc) return rc;
        if (eqstatus_host) HIP_TRY(ctx, hipMemcpyAsync(eqstatus_host + (size_t)done * nc, S.states.get(), (size_t)m * nc, hipMemcpyDeviceToHost, ctx->stream));
        if (weight_host) HIP_TRY(ctx, hipMemcpyAsync(weight_host + done, S.w.get(), sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        done += m;
    }
    return RELMC_OK;
}

int32_t relmc_nsq_is_accumulate(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts, const double* unavail_is,
                                relmc_is_acc* out)
{
    return accumulate_impl(ctx, "relmc_nsq_is_accumulate", seed, first_index, n, opts, unavail_is, out);
}

void relmc_is_acc_zero(relmc_is_acc* acc) { if (acc) std::memset(acc, 0, sizeof(*acc)); }

void relmc_is_acc_merge(relmc_is_acc* d, const relmc_is_acc* s)
{
    if (!d || !s) return;
    d->n += s->n; d->n_fail += s->n_fail; d->n_singular += s->n_singular; d->n_infeasible += s->n_infeasible;
    d->n_nonconverged += s->n_nonconverged; d->sum_iters += s->sum_iters;
    d->sum_w += s->sum_w; d->sum_w2 += s->sum_w2; d->sum_wfail += s->sum_wfail; d->sum_w2fail += s->sum_w2fail;
    d->sum_wdns += s->sum_wdns; d->sum_w2dns2 += s->sum_w2dns2;
    for (int k = 0; k < RELMC_MAX_COMP; ++k) { d->comp_wfail[k] += s->comp_wfail[k]; d->comp_wdns[k] += s->comp_wdns[k]; }
    for (int i = 0; i < RELMC_MAX_BUS; ++i) d->sum_wnodal[i] += s->sum_wnodal[i];
}

void relmc_nsq_is_indices(const relmc_is_acc* a, int32_t nb, int32_t ncomp, double hours, relmc_is_indices* out)
{
    if (!a || !out) return;
    std::memset(out, 0, sizeof(*out));
    out->n = a->n;
    if (a->n <= 0) return;
    const double N = (double)a->n;
    out->edns = a->sum_wdns / N;
    out->plc = a->sum_wfail / N;
    out->lole = out->plc * hours;
    out->eens = out->edns * hours;
    out->beta = beta_of(a->sum_wdns, a->sum_w2dns2, N);
    out->beta_plc = beta_of(a->sum_wfail, a->sum_w2fail, N);
    out->mean_iters = (double)a->sum_iters / N;
    out->mean_w = a->sum_w / N;
    out->ess = a->sum_w2 > 0 ? a->sum_w * a->sum_w / a->sum_w2 : 0.0;
    if (nb > RELMC_MAX_BUS) nb = RELMC_MAX_BUS;
    if (ncomp > RELMC_MAX_COMP) ncomp = RELMC_MAX_COMP;
    for (int i = 0; i < nb; ++i) out->nodal_eens[i] = a->sum_wnodal[i] / N;
    for (int k = 0; k < ncomp; ++k) out->comp_importance[k] = a->sum_wfail > 0 ? a->comp_wfail[k] / a->sum_wfail : 0.0;
}

void relmc_is_tune_opts_default(relmc_is_tune_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->seed = 1; o->n_pilot = 20000; o->max_iters = 5; o->final_iters = 2; o->min_elite = 100; o->rho = 0.1; o->objective = 1;
    o->alpha = 1.0; o->q_max = 0.5;
    relmc_solver_opts_default(&o->solver);
}

int32_t relmc_nsq_is_tune(relmc_ctx* ctx, const relmc_is_tune_opts* o, double* q_out, relmc_is_tune_report* rep_out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_nsq_is_tune: no case loaded");
    if (!o || !q_out || o->n_pilot < 1 || o->n_pilot > kIsLaunch || o->max_iters < 1 || o->max_iters > RELMC_IS_TUNE_MAX_PASSES || o->final_iters < 1 ||
        o->min_elite < 1 || !(o->rho > 0.0 && o->rho <= 1.0) || (o->objective != 0 && o->objective != 1) || o->reserved != 0 ||
        !(o->alpha > 0.0 && o->alpha <= 1.0) || !(o->q_max > 0.0 && o->q_max <= 1.0))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_nsq_is_tune: bad options (n_pilot in 1 .. 2^20, max_iters in 1 .. 32, final_iters and min_elite >= 1, rho, alpha and q_max in (0, 1], objective 0 or 1, reserved 0)");
    if (!ctx->case_copy.valid) return fail(ctx, RELMC_ERR_INVALID, "relmc_nsq_is_tune: the context holds no copy of the case");
    const auto t0 = std::chrono::steady_clock::now();
    const int nc = ctx->ncomp, ng = ctx->ng;
    const int64_t np = o->n_pilot;
    const auto& cc = ctx->case_copy;
    const uint32_t* thr = case_thr(ctx);
    relmc_solver_opts so = o->solver;
    so.screen = 0;
    relmc_is_tune_report rep;
    std::memset(&rep, 0, sizeof(rep));
    std::vector<double> p((size_t)nc), q((size_t)nc), w((size_t)np), dns((size_t)np), e((size_t)np), shortfall, S((size_t)nc);
    std::vector<uint8_t> st((size_t)np * nc);
    std::vector<int64_t> rest;
    for (int k = 0; k < nc; ++k) q[k] = p[k] = (double)thr[k] / kTwo32;
    int rc = buffers_ensure(ctx, np, false);
    if (rc) return rc;
    auto& B = ctx->is;
    const int64_t cb = (np + kIsColChunk - 1) / kIsColChunk;
    std::vector<double> col((size_t)cb * nc);
    double ms = 0.0;
    EventPair es, er;
    HIP_TRY(ctx, es.create()); HIP_TRY(ctx, er.create());
    const int64_t want = (int64_t)std::ceil(o->rho * (double)np);
    for (int t = 0; t < o->max_iters && rep.final_passes < o->final_iters; ++t) {
        rc = tilt_upload(ctx, "relmc_nsq_is_tune", q.data());
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(es.a, ctx->stream));
        rc = sample_queue(ctx, o->seed, (uint64_t)t * (uint64_t)np, np, B.states.get(), B.w.get());
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(es.b, ctx->stream));
        rc = mc_simulation_dev_impl(ctx, B.states.get(), np, &so, B.dns.get(), nullptr, nullptr, nullptr, nullptr);
        if (rc) return rc;
        ms += ctx->last_kernel_ms;
        HIP_TRY(ctx, hipMemcpyAsync(st.data(), B.states.get(), st.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(w.data(), B.w.get(), sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(dns.data(), B.dns.get(), sizeof(double) * (size_t)np, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ms += (double)es.ms();
        // elites and their weights (host): a final pass once the failures alone are enough, else the failures plus the largest shortfalls
        int64_t nf = 0;
        for (int64_t i = 0; i < np; ++i) nf += dns[(size_t)i] > 1e-4;
        const bool final_pass = nf >= o->min_elite;
        int64_t n_elite = nf;
        double level = NAN;
        for (int64_t i = 0; i < np; ++i) {
            const bool f = dns[(size_t)i] > 1e-4;
            e[(size_t)i] = !f ? 0.0 : (final_pass && o->objective == 1 ? w[(size_t)i] * dns[(size_t)i] : w[(size_t)i]);
        }
        if (!final_pass && want > nf) {
            shortfall.assign((size_t)np, 0.0); rest.clear();
            for (int64_t i = 0; i < np; ++i) {
                if (dns[(size_t)i] > 1e-4) continue;
                double cap = 0.0;
                for (int g = 0; g < ng; ++g) if (!st[(size_t)i * nc + g]) cap += cc.inj_pmax[g] > 0.0 ? cc.inj_pmax[g] : 0.0;
                shortfall[(size_t)i] = cc.d.total_load - cap;
                rest.push_back(i);
            }
            const size_t add = std::min<size_t>((size_t)(want - nf), rest.size());
            std::stable_sort(rest.begin(), rest.end(), [&](int64_t a, int64_t b) { return shortfall[(size_t)a] > shortfall[(size_t)b]; });   // ties: the lower index
            for (size_t j = 0; j < add; ++j) e[(size_t)rest[j]] = w[(size_t)rest[j]];
            if (add) level = shortfall[(size_t)rest[add - 1]];
            n_elite += (int64_t)add;
        }
        double sum_e = 0.0;
        for (int64_t i = 0; i < np; ++i) sum_e += e[(size_t)i];
        rep.n_fail[t] = nf; rep.n_elite[t] = n_elite; rep.sum_e[t] = sum_e; rep.level[t] = level;
        rep.passes = t + 1; rep.final_passes += final_pass ? 1 : 0;
        if (!(sum_e > 0.0)) continue;                               // no elite of positive weight: q stays
        // v_k = sum e_i x_ik / sum e_i, the column sums on the device
        HIP_TRY(ctx, hipMemcpyAsync(B.e.get(), e.data(), sizeof(double) * (size_t)np, hipMemcpyHostToDevice, ctx->stream));
        HIP_TRY(ctx, hipEventRecord(er.a, ctx->stream));
        rc = colsum_queue<uint8_t>(ctx, B.states.get(), nc, B.e.get(), np, B.part_col.get());
        if (rc) return rc;
        HIP_TRY(ctx, hipEventRecord(er.b, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(col.data(), B.part_col.get(), sizeof(double) * col.size(), hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        ms += (double)er.ms();
        std::fill(S.begin(), S.end(), 0.0);
        colsum_add(col.data(), cb, nc, S.data());
        for (int k = 0; k < nc; ++k) {
            const double v = S[(size_t)k] / sum_e;
            double x = o->alpha * v + (1.0 - o->alpha) * q[(size_t)k];
            if (x > o->q_max) x = o->q_max;
            if (!(x >= p[(size_t)k])) x = p[(size_t)k];
            q[(size_t)k] = cc.always_up[(size_t)k] ? 0.0 : x;
        }
    }
    for (int k = 0; k < nc; ++k) q_out[k] = q[(size_t)k];
    rep.kernel_seconds = ms * 1e-3;
    rep.wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (rep_out) *rep_out = rep;
    ctx->last_kernel_ms = ms;
    return RELMC_OK;
}

void relmc_is_run_opts_default(relmc_is_run_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->beta_limit = 0.0017; o->max_samples = 100000; o->batch = 1000; o->seed = 1; o->hours_per_year = 8760.0;
    relmc_solver_opts_default(&o->solver);
}

int32_t relmc_nsq_is_run(relmc_ctx* ctx, const relmc_is_run_opts* o, relmc_is_run_result* res)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_nsq_is_run: no case loaded");
    if (comm_ranks(ctx) > 1) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_nsq_is_run: single-rank only (the context has a communicator of more than one rank)");
    if (!o || !res || o->batch <= 0 || o->max_samples <= 0) return fail(ctx, RELMC_ERR_INVALID, "relmc_nsq_is_run: bad options");
    { const int rc = tilt_upload(ctx, "relmc_nsq_is_run", o->unavail_is); if (rc) return rc; }   // a bad tilt is refused before the result is touched
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    double beta = INFINITY, kernel_ms = 0.0;
    int64_t done = 0, cp = 0;
    while (beta > o->beta_limit && done < o->max_samples) {
        const int64_t m = o->max_samples - done < o->batch ? o->max_samples - done : o->batch;
        relmc_is_acc part;
        const int rc = accumulate_impl(ctx, "relmc_nsq_is_run", o->seed, (uint64_t)done, m, &o->solver, o->unavail_is, &part);
        if (rc) return rc;
        kernel_ms += ctx->last_kernel_ms;
        relmc_is_acc_merge(&res->acc, &part);
        done += m;
        relmc_nsq_is_indices(&res->acc, ctx->nb, ctx->ncomp, o->hours_per_year, &res->idx);
        beta = res->idx.beta;
        if (cp < o->history_cap) {
            if (o->beta_history) o->beta_history[cp] = res->idx.beta;
            if (o->edns_history) o->edns_history[cp] = res->idx.edns;
            if (o->plc_history) o->plc_history[cp] = res->idx.plc;
        }
        cp++;
    }
    res->checkpoints = cp < o->history_cap ? cp : o->history_cap;
    res->batches = cp;
    res->converged = beta <= o->beta_limit ? 1 : 0;
    res->kernel_seconds = kernel_ms * 1e-3;
    res->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ctx->last_kernel_ms = kernel_ms;
    return RELMC_OK;
}

}  // extern "C"
