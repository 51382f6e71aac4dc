// relmc_seq.hip — the sequential (chronological) HL2 track of /root/reference/Montecarlo_seq/ (seq_mcsampling.m, seq_mcsimulation.m, calnlc.m,
// seqMain.m:85-249) and the HL1 copper-sheet models of GeneratingAdequacy/PowerSystemAdequacy.jl:169-208 (non-sequential) and :214-268 (sequential).
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_seq_kernels.h"
#include "relmc_hl1_chain_kernels.h"
#include "relmc_seq_event_kernels.h"

namespace relmc_host {

namespace {
// The seven instantiations of relmc_hl1_chain_kernels.h's template that this unit launches, by the names of the launches
constexpr auto relmc_hl1_seq_kernel = relmc_hl1_chain_kernel<HL1_CHAIN_SEQ, 0, double* __restrict__>;
template <bool LIST>
constexpr auto relmc_hl1_event_kernel = relmc_hl1_chain_kernel<HL1_CHAIN_EVENTS, LIST, int32_t, unsigned long long* __restrict__, Hl1EventRec* __restrict__,
                                                               long long* __restrict__, const long long* __restrict__, int64_t, int64_t, relmc_hl1_event* __restrict__>;
template <int NL>
constexpr auto relmc_hl1_sweep_kernel = relmc_hl1_chain_kernel<HL1_CHAIN_SWEEP, NL, const Hl1SweepArgs, double* __restrict__>;

// chronology of years [first_year, first_year + n_years) into the caller's device masks dm (n_years * hpy * mw words, every word written)
int seq_sample(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int n_years, uint32_t* dm)
{
    // segments of at most ~48 KB of masks in LDS, and at least ~2 workgroups per CU over the launch (a segment's chains are walked from hour 0: cheap)
    const int hpy = ctx->hseq.hpy, mw = ctx->hseq.mw, cap = (48 * 1024) / (4 * mw) - 64;
    int nseg = (hpy + cap - 1) / cap;
    while ((int64_t)n_years * nseg < 2 * (int64_t)ctx->num_cu && nseg < 16 && hpy / (nseg + 1) >= 256) ++nseg;
    const int seg_len = (hpy + nseg - 1) / nseg;
    nseg = (hpy + seg_len - 1) / seg_len;
    int sl = seg_len;                                            // LDS row stride = 64 / mw (mod 64): conflict-free word-major rows
    while (sl % 64 != (64 / mw) % 64) ++sl;
    hipLaunchKernelGGL(relmc_seq_sampling_kernel, dim3((unsigned)((int64_t)n_years * nseg)), dim3(256), (size_t)sl * mw * sizeof(uint32_t), ctx->stream,
                       ctx->dseq.get(), seed, first_year, nseg, seg_len, sl, dm);
    if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, "seq: sampling launch failed");
    return RELMC_OK;
}
}  // namespace

int hl1_units_fill(relmc_ctx* ctx, const char* who, int ngen, const double* capacity_mw, const double* mttf_h, const double* mttr_h,
                   double* cap, double* mttf, double* mttr, double* q)
{
    for (int g = 0; g < ngen; ++g) {
        if (!std::isfinite(capacity_mw[g])) return fail(ctx, RELMC_ERR_INVALID, std::string(who) + ": capacity of unit " + std::to_string(g) + " not finite");
        if (!(std::isfinite(mttf_h[g]) && mttf_h[g] > 0.0 && std::isfinite(mttr_h[g]) && mttr_h[g] > 0.0))
            return fail(ctx, RELMC_ERR_INVALID, std::string(who) + ": MTTF / MTTR of unit " + std::to_string(g) + " not finite and positive");
        cap[g] = capacity_mw[g]; mttf[g] = mttf_h[g]; mttr[g] = mttr_h[g];
        q[g] = mttr_h[g] / (mttf_h[g] + mttr_h[g]);
    }
    return RELMC_OK;
}

int hl1_reduce_queue(relmc_ctx* ctx, const char* who, const double* rec, int64_t n, int rows, double* dpart, std::vector<double>& part)
{
    const int64_t blocks = hl1_reduce_blocks(n);
    for (int r = 0; r < rows; ++r)
        hipLaunchKernelGGL(relmc_hl1_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, rec + (size_t)r * n * 3, n,
                           dpart + (size_t)r * blocks * 6);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, std::string(who) + ": launch failed");
    part.resize((size_t)blocks * 6 * rows);
    HIP_TRY(ctx, hipMemcpyAsync(part.data(), dpart, sizeof(double) * part.size(), hipMemcpyDeviceToHost, ctx->stream));
    return RELMC_OK;
}

// The body of relmc_seq_years (arguments checked by the entry): the step that relmc_seq_years and relmc_seq_events share.  It leaves the
// years' per-hour curtailment in ctx->sq.curt and their masks in ctx->sq.dm, and the kernels' time in ctx->last_kernel_ms.
int seq_years_step(relmc_ctx* ctx, const std::string& who, uint64_t seed, uint64_t first_year, int32_t n_years, const relmc_solver_opts* opts,
                   double curtail_threshold, relmc_seq_year* years_out, relmc_acc* acc_out)
{
    relmc_acc_zero(acc_out);
    if (n_years == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const relmc_solver_opts o = solver_opts_or_default(opts);
    const int hpy = ctx->hseq.hpy;
    // the device buffers of a step live in the context and only ever grow
    const size_t nh = (size_t)n_years * hpy, words = nh * (size_t)ctx->hseq.mw;
    auto& Q = ctx->sq;
    // counts: [0, n) listed hours per year, [n, 2 n) contingency hours per year (pre-screen), n = the years the buffer was made for
    if (Q.dm.grow(words) != hipSuccess || Q.hours.grow(nh) != hipSuccess || Q.curt.grow(nh) != hipSuccess || Q.counts.grow(2 * (size_t)n_years) != hipSuccess ||
        Q.off.grow((size_t)n_years + 1) != hipSuccess || Q.year.grow(3 * (size_t)n_years) != hipSuccess)
        return fail(ctx, RELMC_ERR_HIP, who + ": device allocation failed");
    uint32_t* const dm = Q.dm.get(); uint16_t* const dhours = Q.hours.get(); uint32_t* const dcounts = Q.counts.get(); uint32_t* const doff = Q.off.get();
    double* const dcurt = Q.curt.get(); double* const dyear = Q.year.get();
    int rc = seq_sample(ctx, seed, first_year, n_years, dm);
    if (rc) return rc;
    std::vector<uint32_t> counts(n_years), ncont(n_years), off(n_years + 1, 0);
    bool ok = hipMemsetAsync(dcurt, 0, nh * sizeof(double), ctx->stream) == hipSuccess;
    // screen = 1 (relmc_screen.hip): the contingency hours are counted as before, but only the ones the zero-curtailment certificate does not cover
    // -- at the hour's own load factor -- are listed for the interior point; a covered hour's curtailment stays the 0 it was set to above
    const bool screen = screen_active(ctx, o);
    uint32_t* const dncont = dcounts + Q.counts.size() / 2;
    if (screen) ok = ok && screen_seq_compact(ctx, dm, n_years, dhours, dcounts, dncont) == RELMC_OK;
    else hipLaunchKernelGGL(relmc_seq_compact_kernel, dim3(n_years), dim3(256), 0, ctx->stream, dm, hpy, ctx->hseq.mw, dhours, dcounts);
    ok = ok && hipGetLastError() == hipSuccess && hipMemcpyAsync(counts.data(), dcounts, sizeof(uint32_t) * n_years, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess &&
         (!screen || hipMemcpyAsync(ncont.data(), dncont, sizeof(uint32_t) * n_years, hipMemcpyDeviceToHost, ctx->stream) == hipSuccess) &&
         hipStreamSynchronize(ctx->stream) == hipSuccess;
    if (!ok) return fail(ctx, RELMC_ERR_HIP, who + ": compaction failed");
    int64_t certified = 0;
    for (int y = 0; y < n_years; ++y) {
        off[y + 1] = off[y] + counts[y];
        years_out[y].n_contingency = screen ? ncont[y] : counts[y];
        if (screen) certified += (int64_t)ncont[y] - (int64_t)counts[y];
    }
    const int64_t nlp = off[n_years];
    double ms = 0.0;
    if (screen) { float t = 0.f; if (hipEventElapsedTime(&t, ctx->screen_ev0, ctx->screen_ev1) == hipSuccess) ms += t; }      // the certificate's pre-pass (the stream was synchronised above)
    if (nlp > 0) {
        if (hipMemcpyAsync(doff, off.data(), sizeof(uint32_t) * (n_years + 1), hipMemcpyHostToDevice, ctx->stream) != hipSuccess) return fail(ctx, RELMC_ERR_HIP, who + ": H2D failed");
        EvalArgs a = make_args(o);
        a.fail_threshold = curtail_threshold;
        a.n = nlp; a.seq_masks = dm; a.seq_offsets = doff; a.seq_hours = dhours; a.load_factors = ctx->dlf.get(); a.curt = dcurt;
        a.seq_nyears = n_years; a.seq_hpy = hpy;
        Collected c;
        rc = eval_collect(ctx, who.c_str(), 2, a, 0, a.n, acc_out, c);
        if (rc) return rc;
        ms += c.ms;
        RetryOut ro;                                                   // hours the primary elimination order did not converge on
        const ScaleFn scale = [&](unsigned long long u) { return ctx->hlf[(size_t)(u % (unsigned long long)hpy)]; };
        rc = fail_retry(ctx, o, curtail_threshold, &scale, ro, &ms, c.known());
        if (rc) return rc;
        acc_add_retry(acc_out, ro, ctx->ncomp, curtail_threshold);
        for (size_t r = 0; r < ro.size(); ++r) {
            const RetryUnit u = ro[r];
            if (hipMemcpy(dcurt + u.unit, &u.dns, sizeof(double), hipMemcpyHostToDevice) != hipSuccess) return fail(ctx, RELMC_ERR_HIP, who + ": H2D failed");
        }
    }
    acc_out->n += certified; acc_out->n_screened += certified;
    hipLaunchKernelGGL(relmc_seq_annual_kernel, dim3(n_years), dim3(256), 0, ctx->stream, dcurt, hpy, curtail_threshold, dyear);
    std::vector<double> yr((size_t)3 * n_years);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(yr.data(), dyear, sizeof(double) * 3 * n_years, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess ||
        hipStreamSynchronize(ctx->stream) != hipSuccess) return fail(ctx, RELMC_ERR_HIP, who + ": annual indices failed");
    for (int y = 0; y < n_years; ++y) { years_out[y].ens = yr[3 * y]; years_out[y].dlc = yr[3 * y + 1]; years_out[y].nlc = yr[3 * y + 2]; }
    ctx->last_kernel_ms = ms;
    return RELMC_OK;
}

int seq_events_device(relmc_ctx* ctx, const char* who_, const double* curt, const uint32_t* masks, int n_years, int hpy, int mw, double threshold,
                      int64_t total_hint, relmc_seq_event_acc* ev_acc, int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap,
                      relmc_seq_event* events_host, double* ms)
{
    static_assert(SEQ_NCOMPMAX == RELMC_MAX_COMP && SEQ_NCOMPMAX == 256, "one lane of relmc_seq_event_comp_kernel per component");
    static_assert(offsetof(relmc_seq_event_acc, onset_events) + sizeof(SeqEventComp) == sizeof(relmc_seq_event_acc) &&
                  offsetof(relmc_seq_event_acc, involved_energy) - offsetof(relmc_seq_event_acc, onset_events) == offsetof(SeqEventComp, involved_energy),
                  "SeqEventComp is the tail of relmc_seq_event_acc");
    const std::string who(who_);
    ev_acc->years = n_years;
    if (n_years == 0) return RELMC_OK;
    // the targets of the queued copies, and behind them a guard that waits for the stream on an early return, so that no copy is left
    // pending into storage that has gone (it is destroyed first)
    long long total = total_hint, dev_total = -1;
    std::vector<SeqEventPart> part;
    struct Drain { hipStream_t s; bool armed; ~Drain() { if (armed) (void)hipStreamSynchronize(s); } } drain{ctx->stream, true};
    auto& E = ctx->sq_events;
    HIP_TRY(ctx, E.count.grow((size_t)n_years + 1));
    HIP_TRY(ctx, E.offset.grow((size_t)n_years + 1));
    long long* const dcount = E.count.get(); long long* const doff = E.offset.get();
    // count[n_years] = 0, so that the scan of n_years + 1 counts leaves the total in offset[n_years]
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    HIP_TRY(ctx, hipMemsetAsync(dcount + n_years, 0, sizeof(long long), ctx->stream));
    hipLaunchKernelGGL(relmc_seq_event_count_kernel, dim3(n_years), dim3(256), 0, ctx->stream, curt, hpy, threshold, dcount);
    hipLaunchKernelGGL(relmc_hl1_event_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, (const long long*)dcount, (int64_t)n_years + 1, doff);
    if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, who + ": launch failed");
    if (total < 0) {
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        HIP_TRY(ctx, hipMemcpyAsync(&total, doff + n_years, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
        if (finish_timing(ctx) != RELMC_OK) return fail(ctx, RELMC_ERR_HIP, who + ": synchronisation failed");
        *ms += ctx->last_kernel_ms;
        (void)hipEventRecord(ctx->ev0, ctx->stream);
    }
    const int64_t blocks = total > 0 ? hl1_reduce_blocks(total) : 0;
    const int64_t want = events_host ? std::min<int64_t>(total, events_cap) : 0;
    unsigned long long* dhist = nullptr;
    if (total > 0) {
        HIP_TRY(ctx, E.list.grow((size_t)total));
        HIP_TRY(ctx, E.part.grow((size_t)blocks));
        HIP_TRY(ctx, E.comp.grow(1));
        if (dur_hist_host) {
            HIP_TRY(ctx, E.hist.grow((size_t)n_dur_bins));
            dhist = E.hist.get();
            HIP_TRY(ctx, hipMemsetAsync(dhist, 0, sizeof(unsigned long long) * n_dur_bins, ctx->stream));
        }
        hipLaunchKernelGGL(relmc_seq_event_fill_kernel, dim3(n_years), dim3(256), 0, ctx->stream, curt, masks, hpy, mw, threshold, (const long long*)doff,
                           total, E.list.get());
        hipLaunchKernelGGL(relmc_seq_event_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, (const relmc_seq_event*)E.list.get(),
                           (const long long*)(doff + n_years), total, dhist ? n_dur_bins : 0, dhist, E.part.get());
        hipLaunchKernelGGL(relmc_seq_event_comp_kernel, dim3(1), dim3(256), 0, ctx->stream, (const relmc_seq_event*)E.list.get(), (const long long*)(doff + n_years), total,
                           E.comp.get());
        if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, who + ": launch failed");
    }
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    part.resize((size_t)blocks);
    HIP_TRY(ctx, hipMemcpyAsync(&dev_total, doff + n_years, sizeof(long long), hipMemcpyDeviceToHost, ctx->stream));
    if (total > 0) {
        HIP_TRY(ctx, hipMemcpyAsync(part.data(), E.part.get(), sizeof(SeqEventPart) * blocks, hipMemcpyDeviceToHost, ctx->stream));
        HIP_TRY(ctx, hipMemcpyAsync(ev_acc->onset_events, E.comp.get(), sizeof(SeqEventComp), hipMemcpyDeviceToHost, ctx->stream));
        if (dhist) HIP_TRY(ctx, hipMemcpyAsync(dur_hist_host, dhist, sizeof(int64_t) * n_dur_bins, hipMemcpyDeviceToHost, ctx->stream));
        if (want > 0) HIP_TRY(ctx, hipMemcpyAsync(events_host, E.list.get(), sizeof(relmc_seq_event) * want, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (finish_timing(ctx) != RELMC_OK) return fail(ctx, RELMC_ERR_HIP, who + ": synchronisation failed");
    drain.armed = false;
    *ms += ctx->last_kernel_ms;
    if (dev_total != total)
        return fail(ctx, RELMC_ERR_HIP, who + ": " + std::to_string(dev_total) + " loss events on the device, " + std::to_string(total) + " in the annual indices");
    for (const SeqEventPart& p : part) {                     // block by block: the order is part of the results
        ev_acc->events += p.events; ev_acc->censored += p.censored; ev_acc->load_onset_events += p.load_onset;
        ev_acc->sum_dur += p.sum_dur; ev_acc->sum_dur2 += p.sum_dur2; ev_acc->max_dur = std::max<int64_t>(ev_acc->max_dur, p.max_dur);
        ev_acc->sum_energy += p.sum_energy; ev_acc->sum_energy2 += p.sum_energy2;
        ev_acc->max_energy = std::max(ev_acc->max_energy, p.max_energy); ev_acc->max_peak = std::max(ev_acc->max_peak, p.max_peak);
    }
    return RELMC_OK;
}

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

// ---- sequential HL2: Montecarlo_seq/ ---------------------------------------------------------------------
int32_t relmc_seq_load(relmc_ctx* ctx, const double* mttf, const double* mttr, int32_t hpy, const double* load_factors)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_load: no case loaded");
    if (!mttf || !mttr || !load_factors || hpy < 1 || hpy > 65535) return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_load: bad arguments");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    SeqCase& q = ctx->hseq;
    std::memset(&q, 0, sizeof(q));
    if (ctx->ncomp > SEQ_NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_seq_load: more than 256 components");
    q.ncomp = ctx->ncomp; q.hpy = hpy; q.mw = ctx->tile == 0 ? Tile24::OW : Tile96::OW;
    for (int k = 0; k < q.ncomp; ++k) {
        if (!(mttf[k] > 0) || !(mttr[k] > 0)) return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_load: MTTF / MTTR must be positive");
        q.mttf[k] = mttf[k]; q.mttr[k] = mttr[k];
    }
    HIP_TRY(ctx, ctx->dseq.grow(1));
    ctx->dlf.reset();
    HIP_TRY(ctx, ctx->dlf.grow((size_t)hpy));
    ctx->hlf.assign(load_factors, load_factors + hpy);
    HIP_TRY(ctx, hipMemcpy(ctx->dseq.get(), &q, sizeof(q), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->dlf.get(), load_factors, sizeof(double) * hpy, hipMemcpyHostToDevice));
    ctx->has_seq = true;
    return RELMC_OK;
}

int32_t relmc_seq_mcsampling(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t num_years, uint8_t* state_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_mcsampling: relmc_seq_load has not been called");
    if (num_years < 0 || (num_years > 0 && !state_host)) return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_mcsampling: bad arguments");
    if (num_years == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t nh = (int64_t)num_years * ctx->hseq.hpy;
    const size_t bytes = (size_t)nh * ctx->hseq.ncomp;
    DevBuf<uint32_t> dm; DevBuf<uint8_t> dst;
    if (dm.grow((size_t)nh * ctx->hseq.mw) != hipSuccess || dst.grow(bytes) != hipSuccess) return fail(ctx, RELMC_ERR_HIP, "relmc_seq_mcsampling: allocation failed");
    int rc = seq_sample(ctx, seed, first_year, num_years, dm.get());
    if (rc) return rc;
    hipLaunchKernelGGL(relmc_seq_expand_kernel, dim3(ctx->num_cu * 8), dim3(256), 0, ctx->stream, dm.get(), nh, ctx->hseq.ncomp, ctx->hseq.mw, dst.get());
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(state_host, dst.get(), bytes, hipMemcpyDeviceToHost) != hipSuccess) rc = fail(ctx, RELMC_ERR_HIP, "relmc_seq_mcsampling: kernel / copy failed");
    return rc;
}

int32_t relmc_seq_mcsimulation(relmc_ctx* ctx, const uint8_t* states_host, const double* load_scale_host, int64_t n, const relmc_solver_opts* opts,
                               double* dns_host, double* nodal_host, int32_t* status_host, int32_t* iters_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_mcsimulation: no case loaded");
    if (n < 0 || (n > 0 && (!states_host || !dns_host || !load_scale_host))) return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_mcsimulation: bad arguments");
    if (n == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return pipe_run(ctx, states_host, load_scale_host, n, solver_opts_or_default(opts), 0.01 /* CURTAIL_THRESHOLD, seqMain.m:41 */, dns_host, nodal_host, status_host, iters_host);
}

int32_t relmc_seq_years(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t n_years, const relmc_solver_opts* opts,
                        double curtail_threshold, relmc_seq_year* years_out, relmc_acc* acc_out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_years: relmc_seq_load has not been called");
    if (n_years < 0 || !acc_out || (n_years > 0 && !years_out)) return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_years: bad arguments");
    return seq_years_step(ctx, "relmc_seq_years", seed, first_year, n_years, opts, curtail_threshold, years_out, acc_out);
}

// Loss events of the years above: relmc_seq_years' step, then count -> offsets -> fill -> reduce on the curtailment and the masks it left
// on the device.  The years' nlc are the event counts, so the list is sized without reading the device's count back.
int32_t relmc_seq_events(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int32_t n_years, const relmc_solver_opts* opts,
                         double curtail_threshold, relmc_seq_year* years_out, relmc_acc* acc_out, relmc_seq_event_acc* ev_acc,
                         int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap, relmc_seq_event* events_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_events: relmc_seq_load has not been called");
    if (n_years < 0 || !acc_out || !ev_acc || (n_years > 0 && !years_out) || (dur_hist_host && (n_dur_bins < 1 || n_dur_bins > 4096)) || events_cap < 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_events: bad arguments");
    seq_events_zero(ev_acc, n_dur_bins, dur_hist_host);      // here for every return below; seq_events_device adds to them
    int rc = seq_years_step(ctx, "relmc_seq_events", seed, first_year, n_years, opts, curtail_threshold, years_out, acc_out);
    if (rc || n_years == 0) return rc;
    int64_t total = 0;
    for (int y = 0; y < n_years; ++y) total += (int64_t)years_out[y].nlc;
    double ms = ctx->last_kernel_ms;
    rc = seq_events_device(ctx, "relmc_seq_events", ctx->sq.curt.get(), ctx->sq.dm.get(), n_years, ctx->hseq.hpy, ctx->hseq.mw, curtail_threshold, total,
                           ev_acc, n_dur_bins, dur_hist_host, events_cap, events_host, &ms);
    ctx->last_kernel_ms = ms;
    return rc;
}

void relmc_seq_opts_default(relmc_seq_opts* o)
{
    if (!o) return;
    std::memset(o, 0, sizeof(*o));
    o->cov_threshold = 0.05;      /* seqMain.m:40 */
    o->max_years = 4000;          /* seqMain.m:39 */
    o->curtail_threshold = 0.01;  /* seqMain.m:41 */
    o->batch_years = 0;           /* 64 per rank */
    o->seed = 1;
    relmc_solver_opts_default(&o->solver);
}

// seqMain.m:85-199 (the yearly loop with its CoV stop) + :211-249 (LOLE / LOLF, nodal EENS, component importance), single- and multi-rank.
// Years are independent streams keyed by (seed, global year) and every year starts all-up (seqMain.m:91 samples ONE year per call), so the
// years [done, done + m) of a batch are split contiguously over the ranks of the context's communicator; the annual (ens, dlc, nlc) triples are
// all-gathered in year order (a sum all-reduce of a vector in which every rank fills its own slots), every rank walks the same CoV curve
// (:180-185) and stops at the same year (:194); the post-processing accumulators (:146-159) cover exactly the years up to the stopping year --
// the batch it falls into is evaluated again over its used part -- and are all-reduced once per batch.
int32_t relmc_seq_run(relmc_ctx* ctx, const relmc_seq_opts* o, relmc_seq_result* res)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_seq_run: relmc_seq_load has not been called");
    if (!o || !res || o->max_years < 1 || o->batch_years < 0 || !(o->cov_threshold >= 0.0) ||
        ((o->results_year || o->cum_eens || o->cum_cov) && o->years_cap < o->max_years))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_seq_run: bad options (max_years >= 1, batch_years >= 0; history buffers need years_cap >= max_years entries)");
    std::memset(res, 0, sizeof(*res));
    const auto t0 = std::chrono::steady_clock::now();
    const int R = comm_ranks(ctx), r = R > 1 ? ctx->comm_rank : 0;
    const int64_t batch = o->batch_years > 0 ? o->batch_years : (int64_t)64 * R;
    std::vector<double> ens, dlc, nlc, trip;
    std::vector<relmc_seq_year> mine;
    double kernel_ms = 0.0, mean = 0.0, cov = 0.0;
    int64_t done = 0; bool stop = false;
    int64_t n_cont = 0;
    auto eval = [&](int64_t lo, int64_t cnt, relmc_acc* acc) -> int {      // this rank's years [lo, lo + cnt)
        relmc_acc_zero(acc);
        if (cnt <= 0) return RELMC_OK;
        mine.resize((size_t)cnt);
        const int rc = relmc_seq_years(ctx, o->seed, (uint64_t)lo, (int32_t)cnt, &o->solver, o->curtail_threshold, mine.data(), acc);
        if (rc == RELMC_OK) kernel_ms += ctx->last_kernel_ms;
        return rc;
    };
    while (done < o->max_years && !stop) {
        const int64_t m = (o->max_years - done) < batch ? (o->max_years - done) : batch;
        const int64_t lo = done + m * r / R, cnt = done + m * (r + 1) / R - lo;
        relmc_acc acc;
        // what a batch that is cut at the stopping year and taken again must not count twice (as relmc_nsq_run): second attempts, kernel time
        const RetryMark mark(ctx);
        const double kernel_ms0 = kernel_ms;
        int rc = eval(lo, cnt, &acc);
        const std::string local_err = ctx->err;
        // annual triples of the batch in year order on every rank; a rank whose years failed says so with NaNs every rank will see
        trip.assign((size_t)(4 * m), 0.0);
        for (int64_t k = 0; k < cnt; ++k) {
            const size_t q = (size_t)(4 * (lo - done + k));
            if (rc == RELMC_OK) { trip[q] = mine[(size_t)k].ens; trip[q + 1] = mine[(size_t)k].dlc; trip[q + 2] = mine[(size_t)k].nlc; trip[q + 3] = (double)mine[(size_t)k].n_contingency; }
            else trip[q] = trip[q + 1] = trip[q + 2] = trip[q + 3] = NAN;
        }
        if (rc != RELMC_OK && cnt == 0) trip[0] = NAN;
        if (R > 1) {
            const int rc2 = comm_allreduce_f64(ctx, trip.data(), 4 * m);
            if (rc != RELMC_OK) { ctx->err = local_err; return rc; }
            if (rc2) return rc2;
            for (double v : trip) if (v != v) return fail(ctx, RELMC_ERR_HIP, "relmc_seq_run: another rank failed to evaluate its years of the batch (see that rank's relmc_last_error)");
        } else if (rc != RELMC_OK) return rc;
        int64_t used = m;
        for (int64_t k = 0; k < m; ++k) {
            ens.push_back(trip[(size_t)(4 * k)]); dlc.push_back(trip[(size_t)(4 * k + 1)]); nlc.push_back(trip[(size_t)(4 * k + 2)]);
            const size_t y = ens.size();
            double s = 0.0; for (double v : ens) s += v;
            mean = s / (double)y;                                                       // seqMain.m:180
            cov = 0.0;
            if (y > 1) {                                                                // :183-185, std = sample standard deviation
                double ss = 0.0; for (double v : ens) ss += (v - mean) * (v - mean);
                const double sd = std::sqrt(ss / (double)(y - 1));
                cov = sd / (mean * std::sqrt((double)y));                               // all years so far without curtailment: 0 / 0 = NaN, as the reference (:184)
            }
            if (o->results_year) { relmc_seq_year& Y = o->results_year[y - 1]; Y.ens = ens.back(); Y.dlc = dlc.back(); Y.nlc = nlc.back(); Y.n_contingency = (int64_t)trip[(size_t)(4 * k + 3)]; }
            if (o->cum_eens) o->cum_eens[y - 1] = mean;
            if (o->cum_cov) o->cum_cov[y - 1] = cov;
            n_cont += (int64_t)trip[(size_t)(4 * k + 3)];
            if (y > 1 && cov < o->cov_threshold && cov > 0.0) { stop = true; used = k + 1; break; }      // :194
        }
        if (used < m) {
            // the reference stops inside this batch: its accumulators (seqMain.m:146-159) hold the years up to the stopping year only
            const int64_t hi = done + used;
            const int64_t cnt2 = (lo + cnt < hi ? lo + cnt : hi) - lo;
            // the discarded pass leaves no trace in the bookkeeping: kernel_seconds and relmc_retry_stats do not depend on batch_years
            mark.restore(ctx);
            kernel_ms = kernel_ms0;
            rc = eval(lo, cnt2 > 0 ? cnt2 : 0, &acc);
        }
        if (R > 1) {
            const std::string e2 = ctx->err;
            if (rc != RELMC_OK) { relmc_acc_zero(&acc); acc.n_nonconverged = -((int64_t)1 << 40); }
            const int rc2 = relmc_comm_allreduce_acc(ctx, &acc);
            if (rc != RELMC_OK) { ctx->err = e2; return rc; }
            if (rc2) return rc2;
            if (acc.n_nonconverged < 0) return fail(ctx, RELMC_ERR_HIP, "relmc_seq_run: another rank failed to re-evaluate its years up to the stopping year");
        } else if (rc != RELMC_OK) return rc;
        relmc_acc_merge(&res->acc, &acc);
        done += used;
    }
    const int64_t Y = (int64_t)ens.size();
    res->final_year = (int32_t)Y; res->converged = stop ? 1 : 0;
    res->eens = mean; res->cov = cov;
    double sd = 0.0, sn = 0.0; for (int64_t k = 0; k < Y; ++k) { sd += dlc[(size_t)k]; sn += nlc[(size_t)k]; }
    res->lole = sd / (double)Y; res->lolf = sn / (double)Y;                             // :212-213
    res->plc = sd / ((double)Y * (double)ctx->hseq.hpy);
    res->n_contingency = n_cont;
    for (int i = 0; i < ctx->nb; ++i) res->nodal_eens_avg[i] = res->acc.sum_nodal[i] / (double)Y;                                        // :218
    for (int k = 0; k < ctx->ncomp; ++k) res->comp_importance[k] = res->acc.n_fail ? (double)res->acc.comp_fail[k] / (double)res->acc.n_fail : 0.0;   // :233
    res->kernel_seconds = kernel_ms * 1e-3;
    res->wall_seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    ctx->last_kernel_ms = kernel_ms;
    return RELMC_OK;
}

// ---- HL1 copper sheet: PowerSystemAdequacy.jl:169-208 --------------------------------------------------
int32_t relmc_hl1_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* for_rate, int32_t nhours,
                       const double* hourly_load_mw)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!capacity_mw || !for_rate || !hourly_load_mw || ngen < 1 || nhours < 1) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_load: bad arguments");
    if (ngen > NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_load: more than 128 units");
    Hl1Case h; std::memset(&h, 0, sizeof(h));
    h.ngen = ngen; h.nhours = nhours;
    for (int g = 0; g < ngen; ++g) {
        const std::string unit = " of unit " + std::to_string(g);
        if (!std::isfinite(capacity_mw[g])) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_load: capacity" + unit + " not finite");
        if (!(for_rate[g] >= 0.0 && for_rate[g] <= 1.0)) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_load: for_rate" + unit + " not in [0, 1]");
        double t = std::floor(for_rate[g] * 4294967296.0);
        if (t > 4294967295.0) t = 4294967295.0;
        h.thr[g] = (uint32_t)t; h.cap[g] = capacity_mw[g];
    }
    if (const int64_t bad = first_non_finite(hourly_load_mw, nhours); bad >= 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_load: load of hour " + std::to_string(bad) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // suffix[2k], suffix[2k + 1] = sum(sorted[k:]) as a double-double (hi, lo): the kernel's EUE = suffix - cap * hours cancels when the
    // loads above cap lie close to it, so the sum must carry more than 53 bits (TwoSum per term, then renormalised)
    std::vector<double> sorted(hourly_load_mw, hourly_load_mw + nhours), suffix(2 * (size_t)nhours + 2, 0.0);
    std::sort(sorted.begin(), sorted.end());
    for (int k = nhours - 1; k >= 0; --k) {
        const double a = suffix[2 * k + 2], b = sorted[k], s = a + b, bb = s - a, e = (a - (s - bb)) + (b - bb);
        const double lo = suffix[2 * k + 3] + e, hi = s + lo;
        suffix[2 * k] = hi; suffix[2 * k + 1] = lo - (hi - s);
    }
    auto& H = ctx->hl1;
    H.sorted.reset(); H.suffix.reset();
    HIP_TRY(ctx, H.dcase.grow(1));
    HIP_TRY(ctx, H.sorted.grow((size_t)nhours));
    HIP_TRY(ctx, H.suffix.grow(suffix.size()));
    HIP_TRY(ctx, hipMemcpy(ctx->hl1.dcase.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->hl1.sorted.get(), sorted.data(), sizeof(double) * nhours, hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(ctx->hl1.suffix.get(), suffix.data(), sizeof(double) * suffix.size(), hipMemcpyHostToDevice));
    ctx->hl1_hours = nhours; ctx->has_hl1 = true;
    return RELMC_OK;
}

int32_t relmc_hl1_nsq(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, relmc_hl1_acc* acc, double* iter_lole_host,
                      double* iter_eue_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_nsq: relmc_hl1_load has not been called");
    if (n < 0 || !acc) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_nsq: bad arguments");
    std::memset(acc, 0, sizeof(*acc));
    if (n == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    int64_t blocks = (n + 255) / 256;
    if (blocks > (int64_t)ctx->num_cu * 8) blocks = (int64_t)ctx->num_cu * 8;
    // per-iteration outputs and block partials live in the context between calls (three hipMalloc / hipFree pairs were 0.5 ms of a 0.8 ms call)
    auto& H = ctx->hl1;
    if (iter_lole_host || iter_eue_host) { HIP_TRY(ctx, H.lole.grow((size_t)n)); HIP_TRY(ctx, H.eue.grow((size_t)n)); }
    HIP_TRY(ctx, H.part.grow(4 * (size_t)blocks));
    double* const dl = iter_lole_host ? ctx->hl1.lole.get() : nullptr; double* const de = iter_eue_host ? ctx->hl1.eue.get() : nullptr; double* const dpart = ctx->hl1.part.get();
    int rc = RELMC_OK;
    (void)hipEventRecord(ctx->ev0, ctx->stream);
    hipLaunchKernelGGL(relmc_hl1_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, ctx->hl1.dcase.get(), ctx->hl1.sorted.get(), ctx->hl1.suffix.get(), seed,
                       first_index, n, dl, de, dpart);
    (void)hipEventRecord(ctx->ev1, ctx->stream);
    std::vector<double> part((size_t)4 * blocks);
    if (hipGetLastError() != hipSuccess || hipMemcpyAsync(part.data(), dpart, sizeof(double) * 4 * blocks, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess)
        rc = fail(ctx, RELMC_ERR_HIP, "relmc_hl1_nsq: launch failed");
    if (rc == RELMC_OK && iter_lole_host && hipMemcpyAsync(iter_lole_host, dl, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, RELMC_ERR_HIP, "relmc_hl1_nsq: D2H failed");
    if (rc == RELMC_OK && iter_eue_host && hipMemcpyAsync(iter_eue_host, de, sizeof(double) * n, hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) rc = fail(ctx, RELMC_ERR_HIP, "relmc_hl1_nsq: D2H failed");
    if (rc == RELMC_OK && finish_timing(ctx) != RELMC_OK) rc = fail(ctx, RELMC_ERR_HIP, "relmc_hl1_nsq: synchronisation failed");
    if (rc) return rc;
    acc->n = n;
    for (int64_t b = 0; b < blocks; ++b) { acc->sum_lole += part[4 * b]; acc->sum_eue += part[4 * b + 1]; acc->sum_lole2 += part[4 * b + 2]; acc->sum_eue2 += part[4 * b + 3]; }
    return RELMC_OK;
}

// ---- HL1 sequential chronology: PowerSystemAdequacy.jl:214-268 ----------------------------------------------------------------
int32_t relmc_hl1_seq_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* mttf_h, const double* mttr_h,
                           int32_t nhours, const double* hourly_load_mw)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!capacity_mw || !mttf_h || !mttr_h || !hourly_load_mw || ngen < 1 || nhours < 1)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_load: bad arguments");
    if (ngen > NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_seq_load: more than 128 units");
    Hl1SeqCase h; std::memset(&h, 0, sizeof(h));
    h.ngen = ngen; h.nhours = nhours;
    if (const int rc = hl1_units_fill(ctx, "relmc_hl1_seq_load", ngen, capacity_mw, mttf_h, mttr_h, h.cap, h.mttf, h.mttr, h.q)) return rc;
    if (const int64_t bad = first_non_finite(hourly_load_mw, nhours); bad >= 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_load: load of hour " + std::to_string(bad) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_seq;
    ctx->has_hl1_seq = false;
    HIP_TRY(ctx, S.dcase.grow(1));
    HIP_TRY(ctx, S.load.grow((size_t)nhours));
    HIP_TRY(ctx, hipMemcpy(S.dcase.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.load.get(), hourly_load_mw, sizeof(double) * nhours, hipMemcpyHostToDevice));
    S.ngen = ngen; S.nhours = nhours; ctx->has_hl1_seq = true;
    return RELMC_OK;
}

int32_t relmc_hl1_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                      relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_seq: relmc_hl1_seq_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq: bad arguments");
    std::memset(acc, 0, sizeof(*acc));
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_seq;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int rc = hl1_run_records(ctx, "relmc_hl1_seq", S.rec, n_chains, hl1_chunk_items(n_chains, kHl1RecordBudget, years_per_chain), years_per_chain, 1, sum,
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(relmc_hl1_seq_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, S.rec.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) -> int {
            if (years_host)
                HIP_TRY(ctx, hipMemcpyAsync(years_host + c0 * years_per_chain, S.rec.years.get(), sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        hl1_no_host_step);
    if (rc) return rc;
    hl1_acc_fill(acc, n_chains * years_per_chain, sum);
    return RELMC_OK;
}

// Loss events of the chronology above: per chunk of chains one launch for the chain records, the counts and the histogram and one for
// their fixed-order reduction; when a list is wanted and not yet full, a scan of the counts and a second walk of the chains that writes
// each chain's events at its offset (no per-chain cap, no atomics on the list, step order inside a chain).
int32_t relmc_hl1_seq_events(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                             relmc_hl1_event_acc* acc, int32_t n_dur_bins, int64_t* dur_hist_host, int64_t events_cap, relmc_hl1_event* events_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_seq_events: relmc_hl1_seq_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start) || (dur_hist_host && (n_dur_bins < 1 || n_dur_bins > 4096)) || events_cap < 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_events: bad arguments");
    std::memset(acc, 0, sizeof(*acc));
    if (dur_hist_host) std::memset(dur_hist_host, 0, sizeof(int64_t) * n_dur_bins);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_seq;
    auto& E = ctx->hl1_events;
    // the chunks of relmc_hl1_seq: at most ~4M chain years per launch; a chain's events never depend on the launch it is in
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, years_per_chain);
    const int64_t pblocks = hl1_reduce_blocks(per);
    HIP_TRY(ctx, E.rec.grow((size_t)per));
    HIP_TRY(ctx, E.count.grow((size_t)per));
    HIP_TRY(ctx, E.part.grow((size_t)pblocks));
    unsigned long long* dhist = nullptr;
    if (dur_hist_host) {
        HIP_TRY(ctx, E.hist.grow((size_t)n_dur_bins));
        dhist = E.hist.get();
        HIP_TRY(ctx, hipMemsetAsync(dhist, 0, sizeof(unsigned long long) * n_dur_bins, ctx->stream));
    }
    std::vector<Hl1EventRec> part;
    Hl1EventRec sum; std::memset(&sum, 0, sizeof(sum));
    double kernel_ms = 0.0;
    int64_t listed = 0;
    for (int64_t c0 = 0; c0 < n_chains; c0 += per) {
        const int64_t nc = std::min(per, n_chains - c0), blocks = hl1_reduce_blocks(nc);
        const dim3 grid((unsigned)((nc + 3) / 4));
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        hipLaunchKernelGGL(relmc_hl1_event_kernel<false>, grid, dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                           first_chain + (uint64_t)c0, nc, years_per_chain, start, dur_hist_host ? n_dur_bins : 0, dhist, E.rec.get(), E.count.get(),
                           (const long long*)nullptr, c0, (int64_t)0, (relmc_hl1_event*)nullptr);
        hipLaunchKernelGGL(relmc_hl1_event_reduce_kernel, dim3((unsigned)blocks), dim3(256), 0, ctx->stream, E.rec.get(), nc, E.part.get());
        (void)hipEventRecord(ctx->ev1, ctx->stream);
        if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, "relmc_hl1_seq_events: launch failed");
        part.resize((size_t)blocks);
        HIP_TRY(ctx, hipMemcpyAsync(part.data(), E.part.get(), sizeof(Hl1EventRec) * blocks, hipMemcpyDeviceToHost, ctx->stream));
        if (finish_timing(ctx) != RELMC_OK) return fail(ctx, RELMC_ERR_HIP, "relmc_hl1_seq_events: synchronisation failed");
        kernel_ms += ctx->last_kernel_ms;
        int64_t chunk_events = 0;
        for (const Hl1EventRec& p : part) {                  // block by block: the order is part of the results
            chunk_events += p.events;
            sum.events += p.events; sum.sum_dur += p.sum_dur; sum.sum_dur2 += p.sum_dur2; sum.censored += p.censored;
            sum.max_dur = std::max(sum.max_dur, p.max_dur);
            sum.sum_energy += p.sum_energy; sum.sum_energy2 += p.sum_energy2;
            sum.max_energy = std::max(sum.max_energy, p.max_energy); sum.max_peak = std::max(sum.max_peak, p.max_peak);
        }
        const int64_t want = events_host ? std::min(chunk_events, events_cap - listed) : 0;
        if (want > 0) {
            HIP_TRY(ctx, E.offset.grow((size_t)per));
            HIP_TRY(ctx, E.list.grow((size_t)want));
            (void)hipEventRecord(ctx->ev0, ctx->stream);
            hipLaunchKernelGGL(relmc_hl1_event_scan_kernel, dim3(1), dim3(256), 0, ctx->stream, E.count.get(), nc, E.offset.get());
            hipLaunchKernelGGL(relmc_hl1_event_kernel<true>, grid, dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, 0, (unsigned long long*)nullptr, (Hl1EventRec*)nullptr,
                               (long long*)nullptr, (const long long*)E.offset.get(), c0, want, E.list.get());
            (void)hipEventRecord(ctx->ev1, ctx->stream);
            if (hipGetLastError() != hipSuccess) return fail(ctx, RELMC_ERR_HIP, "relmc_hl1_seq_events: launch failed");
            HIP_TRY(ctx, hipMemcpyAsync(events_host + listed, E.list.get(), sizeof(relmc_hl1_event) * want, hipMemcpyDeviceToHost, ctx->stream));
            if (finish_timing(ctx) != RELMC_OK) return fail(ctx, RELMC_ERR_HIP, "relmc_hl1_seq_events: synchronisation failed");
            kernel_ms += ctx->last_kernel_ms;
            listed += want;
        }
    }
    if (dur_hist_host) HIP_TRY(ctx, hipMemcpy(dur_hist_host, dhist, sizeof(int64_t) * n_dur_bins, hipMemcpyDeviceToHost));
    ctx->last_kernel_ms = kernel_ms;
    acc->years = n_chains * years_per_chain;
    acc->events = sum.events; acc->censored = sum.censored; acc->sum_dur = sum.sum_dur; acc->sum_dur2 = sum.sum_dur2; acc->max_dur = sum.max_dur;
    acc->sum_energy = sum.sum_energy; acc->sum_energy2 = sum.sum_energy2; acc->max_energy = sum.max_energy; acc->max_peak = sum.max_peak;
    return RELMC_OK;
}

// Load sweep on the chronology above: per chunk of chains one launch that walks every chain once and writes the year records of all
// levels ([level][chain][year][3]), then relmc_hl1_reduce_kernel over each level's slice.  A chunk holds at most ~4M year records over all
// levels; a chain's records never depend on the chunk it is in.
int32_t relmc_hl1_seq_sweep(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                            int32_t n_levels, const relmc_hl1_sweep_level* levels, const uint32_t* withheld, relmc_hl1_seq_acc* acc,
                            relmc_hl1_seq_year* years_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_seq_sweep: relmc_hl1_seq_load has not been called");
    if (!levels || !hl1_chain_args_ok(acc, n_chains, years_per_chain, start))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_sweep: bad arguments");
    if (n_levels < 1 || n_levels > RELMC_HL1_SWEEP_MAX_LEVELS)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_sweep: n_levels " + std::to_string(n_levels) + " not in 1.." + std::to_string(RELMC_HL1_SWEEP_MAX_LEVELS));
    auto& S = ctx->hl1_seq;
    Hl1SweepArgs A; std::memset(&A, 0, sizeof(A));
    A.n_levels = n_levels;
    for (int j = 0; j < n_levels; ++j) {
        const relmc_hl1_sweep_level& v = levels[j];
        const std::string lvl = "relmc_hl1_seq_sweep: level " + std::to_string(j);
        if (!std::isfinite(v.scale) || !std::isfinite(v.shift)) return fail(ctx, RELMC_ERR_INVALID, lvl + ": scale / shift not finite");
        if (v.fleet != 0 && v.fleet != 1) return fail(ctx, RELMC_ERR_INVALID, lvl + ": fleet " + std::to_string(v.fleet) + " is not 0 or 1");
        if (v.reserved != 0) return fail(ctx, RELMC_ERR_INVALID, lvl + ": reserved must be 0");
        if (v.fleet == 1 && !withheld) return fail(ctx, RELMC_ERR_INVALID, lvl + ": fleet 1 without a withheld mask");
        A.lv[j] = v;
        if (v.fleet == 1) A.fleet1 |= 1u << j;
    }
    for (int j = n_levels; j < RELMC_HL1_SWEEP_MAX_LEVELS; ++j) { A.lv[j].scale = 0.0; A.lv[j].shift = -INFINITY; }      // never loses
    if (withheld)
        for (int k = S.ngen; k < 128; ++k)
            if ((withheld[k >> 5] >> (k & 31)) & 1u)
                return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_seq_sweep: withheld bit " + std::to_string(k) + " at or above ngen = " + std::to_string(S.ngen));
    if (withheld) std::memcpy(A.withheld, withheld, sizeof(A.withheld));
    const int64_t total = n_chains * years_per_chain;
    std::memset(acc, 0, sizeof(*acc) * n_levels);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& X = ctx->hl1_sweep;
    const auto kernel = n_levels <= 1 ? relmc_hl1_sweep_kernel<1> : n_levels <= 4 ? relmc_hl1_sweep_kernel<4>
                      : n_levels <= 8 ? relmc_hl1_sweep_kernel<8> : relmc_hl1_sweep_kernel<16>;
    std::vector<double> sum((size_t)6 * n_levels, 0.0);
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * n_levels);      // a chain counts its records of all levels
    const int rc = hl1_run_records(ctx, "relmc_hl1_seq_sweep", X, n_chains, per, years_per_chain, n_levels, sum.data(),
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, A, X.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) -> int {
            if (years_host)
                for (int j = 0; j < n_levels; ++j)
                    HIP_TRY(ctx, hipMemcpyAsync(years_host + (size_t)j * total + c0 * years_per_chain, X.years.get() + (size_t)j * nrec * 3,
                                                sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        hl1_no_host_step);
    if (rc) return rc;
    for (int j = 0; j < n_levels; ++j) hl1_acc_fill(acc + j, total, sum.data() + (size_t)6 * j);
    return RELMC_OK;
}

}  // extern "C"
