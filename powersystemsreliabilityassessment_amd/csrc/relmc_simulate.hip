// relmc_simulate.hip — mc_simulation over host or device buffers (mc_simulation.m:1, batched like the parfor of nsqMain.m:257-263) and the fused
// sample -> evaluate -> reduce pass (relmc_nsq_accumulate); the nsqMain loop around it is relmc_nsq_run.hip.
#include <cmath>
#include <cstring>
#include <thread>

#include "relmc_ctx.h"

namespace relmc_host {

// ---- host-buffer evaluation: states in pageable host memory -> dns / nodal / status / iterations in host memory ---------
// What a MATLAB / Julia / Python caller of mc_simulation hands over.  The range is cut into chunks of kPipeChunk states that
// run through a double-buffered pipeline on three streams (H2D, kernel, D2H) with pinned staging buffers; the host copies
// chunk k in and chunk k-2 out while the GPU works on chunk k-1.  Device and staging buffers are allocated once per context.
constexpr int64_t kPipeChunk = 131072;

int pipe_ensure(relmc_ctx* ctx)
{
    auto& P = ctx->pipe;
    if (P.ready && P.ncomp == ctx->ncomp && P.nb == ctx->nb) return RELMC_OK;
    P.ready = false;
    if (!P.up) HIP_TRY(ctx, hipStreamCreateWithFlags(&P.up, hipStreamNonBlocking));
    if (!P.down) HIP_TRY(ctx, hipStreamCreateWithFlags(&P.down, hipStreamNonBlocking));
    for (int b = 0; b < 2; ++b)
        for (hipEvent_t* e : {&P.e_up[b], &P.e_ks[b], &P.e_ke[b], &P.e_down[b]}) if (!*e) HIP_TRY(ctx, hipEventCreate(e));
    const size_t c = (size_t)kPipeChunk, nc = (size_t)ctx->ncomp, nb = (size_t)ctx->nb;
    bool ok = true;
    for (auto& B : P.buf) {
        B = {};                  // sized for the case's component and bus counts: rebuilt when they change
        ok = ok && B.d_st.grow(c * nc) == hipSuccess && B.d_sc.grow(c) == hipSuccess && B.d_dns.grow(c) == hipSuccess && B.d_nod.grow(c * nb) == hipSuccess &&
             B.d_stat.grow(c) == hipSuccess && B.d_it.grow(c) == hipSuccess && B.h_st.grow(c * nc) == hipSuccess && B.h_sc.grow(c) == hipSuccess &&
             B.h_dns.grow(c) == hipSuccess && B.h_nod.grow(c * nb) == hipSuccess && B.h_stat.grow(c) == hipSuccess && B.h_it.grow(c) == hipSuccess;
    }
    if (!ok) { for (auto& B : P.buf) B = {}; return fail(ctx, RELMC_ERR_HIP, "host-buffer pipeline: allocation failed"); }
    P.ready = true; P.ncomp = ctx->ncomp; P.nb = ctx->nb;
    return RELMC_OK;
}

// memcpy spread over a few threads: one core moves ~8 GB/s, the nodal output of 1e6 states is 200 MB
void par_memcpy(void* dst, const void* src, size_t bytes)
{
    const size_t kMin = (size_t)4 << 20;
    int nt = bytes / kMin > 4 ? 4 : (int)(bytes / kMin);
    if (nt <= 1) { std::memcpy(dst, src, bytes); return; }
    std::vector<std::thread> th;
    const size_t per = ((bytes / nt) + 63) & ~(size_t)63;
    for (int t = 1; t < nt; ++t) {
        const size_t off = per * t, len = t == nt - 1 ? bytes - off : per;
        th.emplace_back([=]() { std::memcpy((char*)dst + off, (const char*)src + off, len); });
    }
    std::memcpy(dst, src, per);
    for (auto& t : th) t.join();
}

int pipe_run(relmc_ctx* ctx, const uint8_t* states, const double* load_scale, int64_t n, const relmc_solver_opts& o, double fail_threshold,
             double* dns, double* nodal, int32_t* status, int32_t* iters)
{
    int rc = pipe_ensure(ctx);
    if (rc) return rc;
    auto& P = ctx->pipe;
    const size_t nc = (size_t)ctx->ncomp, nb = (size_t)ctx->nb;
    const int64_t nchunk = (n + kPipeChunk - 1) / kPipeChunk;
    double kernel_ms = 0.0;
    auto drain = [&](int64_t k) -> int {                      // chunk k's results: wait for its D2H, copy out of the staging buffers
        const int b = (int)(k & 1);
        const int64_t lo = k * kPipeChunk, m = (n - lo) < kPipeChunk ? (n - lo) : kPipeChunk;
        HIP_TRY(ctx, hipEventSynchronize(P.e_down[b]));
        float ms = 0.f;
        if (hipEventElapsedTime(&ms, P.e_ks[b], P.e_ke[b]) == hipSuccess) kernel_ms += ms;
        std::memcpy(dns + lo, P.buf[b].h_dns.get(), sizeof(double) * (size_t)m);
        if (nodal) par_memcpy(nodal + (size_t)lo * nb, P.buf[b].h_nod.get(), sizeof(double) * (size_t)m * nb);
        if (status) std::memcpy(status + lo, P.buf[b].h_stat.get(), sizeof(int32_t) * (size_t)m);
        if (iters) std::memcpy(iters + lo, P.buf[b].h_it.get(), sizeof(int32_t) * (size_t)m);
        return RELMC_OK;
    };
    for (int64_t k = 0; k < nchunk; ++k) {
        const int b = (int)(k & 1);
        const int64_t lo = k * kPipeChunk, m = (n - lo) < kPipeChunk ? (n - lo) : kPipeChunk;
        if (k >= 2) { rc = drain(k - 2); if (rc) return rc; }     // frees slot b (device buffers and staging)
        par_memcpy(P.buf[b].h_st.get(), states + (size_t)lo * nc, (size_t)m * nc);
        if (load_scale) std::memcpy(P.buf[b].h_sc.get(), load_scale + lo, sizeof(double) * (size_t)m);
        HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].d_st.get(), P.buf[b].h_st.get(), (size_t)m * nc, hipMemcpyHostToDevice, P.up));
        if (load_scale) HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].d_sc.get(), P.buf[b].h_sc.get(), sizeof(double) * (size_t)m, hipMemcpyHostToDevice, P.up));
        HIP_TRY(ctx, hipEventRecord(P.e_up[b], P.up));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, P.e_up[b], 0));
        EvalArgs a = make_args(o);
        a.fail_threshold = fail_threshold;
        a.n = m; a.states = P.buf[b].d_st.get(); a.load_scale = load_scale ? P.buf[b].d_sc.get() : nullptr;
        a.dns = P.buf[b].d_dns.get(); a.nodal = nodal ? P.buf[b].d_nod.get() : nullptr; a.status = status ? P.buf[b].d_stat.get() : nullptr; a.iters = iters ? P.buf[b].d_it.get() : nullptr;
        int rows = 0;
        rc = fail_arm(ctx, a, lo, k == 0, n);
        if (rc) return rc;
        rc = launch_eval(ctx, 1, a, &rows, P.e_ks[b], P.e_ke[b]);
        if (rc) return rc;
        HIP_TRY(ctx, hipStreamWaitEvent(P.down, P.e_ke[b], 0));
        HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].h_dns.get(), P.buf[b].d_dns.get(), sizeof(double) * (size_t)m, hipMemcpyDeviceToHost, P.down));
        if (nodal) HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].h_nod.get(), P.buf[b].d_nod.get(), sizeof(double) * (size_t)m * nb, hipMemcpyDeviceToHost, P.down));
        if (status) HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].h_stat.get(), P.buf[b].d_stat.get(), sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, P.down));
        if (iters) HIP_TRY(ctx, hipMemcpyAsync(P.buf[b].h_it.get(), P.buf[b].d_it.get(), sizeof(int32_t) * (size_t)m, hipMemcpyDeviceToHost, P.down));
        HIP_TRY(ctx, hipEventRecord(P.e_down[b], P.down));
    }
    for (int64_t k = nchunk >= 2 ? nchunk - 2 : 0; k < nchunk; ++k) { rc = drain(k); if (rc) return rc; }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    RetryOut ro;
    const ScaleFn scale = [&](unsigned long long u) { return load_scale[u]; };
    rc = fail_retry(ctx, o, fail_threshold, load_scale ? &scale : nullptr, ro, &kernel_ms);
    if (rc) return rc;
    for (size_t r = 0; r < ro.size(); ++r) {                  // the second attempt's results in the place of the first's
        const RetryUnit u = ro[r];
        dns[u.unit] = u.dns;
        if (nodal) std::memcpy(nodal + u.unit * nb, u.nodal, sizeof(double) * nb);
        if (status) status[u.unit] = u.status;
        if (iters) iters[u.unit] = u.iters;
    }
    ctx->last_kernel_ms = kernel_ms;
    return RELMC_OK;
}

// dns_dev (optional, n doubles): dns of every sample of the range in sampling order, beside the accumulators
int nsq_accumulate_impl(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts, relmc_acc* acc_out, double* dns_dev)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_nsq_accumulate: no case loaded");
    if (n < 0 || !acc_out) return fail(ctx, RELMC_ERR_INVALID, "relmc_nsq_accumulate: bad arguments");
    relmc_acc_zero(acc_out);
    if (n == 0) return RELMC_OK;
    const relmc_solver_opts o = solver_opts_or_default(opts);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // a wavefront row counts its scenarios in 32 bits: split very large ranges
    // screen = 1 (relmc_screen.hip): a pre-pass draws the masks and runs the zero-curtailment certificate, one thread per sample; only the samples it
    // does not cover are solved (MODE 7, from the stored masks, in ascending sample order), the others add 1 to n and to n_screened
    const bool screen = screen_active(ctx, o);
    const int64_t kMaxPerLaunch = screen ? kScreenChunk : (int64_t)1 << 31;
    double ms_total = 0.0;
    for (int64_t done = 0; done < n;) {
        const int64_t m = (n - done) < kMaxPerLaunch ? (n - done) : kMaxPerLaunch;
        EvalArgs a = make_args(o);
        a.seed = seed; a.first_index = first_index + (uint64_t)done; a.n = m;
        a.dns = dns_dev ? dns_dev + done : nullptr;
        int64_t certified = 0;
        if (screen) {
            uint32_t ns = 0;
            if (dns_dev) HIP_TRY(ctx, hipMemsetAsync(dns_dev + done, 0, sizeof(double) * (size_t)m, ctx->stream));
            const int rc0 = screen_prepass_nsq(ctx, seed, first_index + (uint64_t)done, m, &ns, &ms_total);
            if (rc0) return rc0;
            certified = m - (int64_t)ns;
            a.n = (int64_t)ns; a.memo_keys = ctx->screen.keys.get(); a.memo_perm = ctx->screen.idx.get();
        }
        relmc_acc part;
        relmc_acc_zero(&part);
        Collected c;
        for (int attempt = 0; a.n > 0; ++attempt) {
            int rc = eval_collect(ctx, "relmc_nsq_accumulate", screen ? 7 : 0, a, done, m, &part, c);
            if (rc) return rc;
            ms_total += c.ms;
            // more non-converged units than the list holds (a case the calibration did not foresee): a longer list and the same chunk again --
            // the launch is a function of (seed, range) alone, so the second one lists them all
            if (!c.armed || c.listed <= ctx->retry.fail.size() || ctx->retry.fail.size() >= kFailCapMax || attempt >= 2) break;
            HIP_TRY(ctx, hipMemset(ctx->retry.fail_count.get(), 0, ctx->retry.kCountBytes));
            rc = fail_list_ensure(ctx, c.listed + c.listed / 8 > kFailCapMax ? kFailCapMax : c.listed + c.listed / 8);
            if (rc) return rc;
        }
        part.n += certified; part.n_screened += certified;
        int rc = RELMC_OK;
        RetryOut ro;
        if (a.n > 0) rc = fail_retry(ctx, o, a.fail_threshold, nullptr, ro, &ms_total, c.known());
        if (rc) return rc;
        acc_add_retry(&part, ro, ctx->ncomp, a.fail_threshold);
        for (size_t r = 0; dns_dev && r < ro.size(); ++r) {
            const RetryUnit u = ro[r];
            HIP_TRY(ctx, hipMemcpy(dns_dev + u.unit, &u.dns, sizeof(double), hipMemcpyHostToDevice));
        }
        relmc_acc_merge(acc_out, &part);
        done += m;
    }
    ctx->last_kernel_ms = ms_total;
    return RELMC_OK;
}

int mc_simulation_dev_impl(relmc_ctx* ctx, const uint8_t* states_dev, int64_t n, const relmc_solver_opts* opts, double* dns_dev, double* nodal_dev,
                           int32_t* status_dev, int32_t* iters_dev, int64_t* n_infeasible_out)
{
    if (n_infeasible_out) *n_infeasible_out = 0;
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_mc_simulation: no case loaded");
    if (n < 0 || (n > 0 && (!states_dev || !dns_dev))) return fail(ctx, RELMC_ERR_INVALID, "relmc_mc_simulation: bad arguments");
    if (n == 0) return RELMC_OK;
    const relmc_solver_opts o = solver_opts_or_default(opts);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    EvalArgs a = make_args(o);
    a.n = n; a.states = states_dev; a.dns = dns_dev; a.nodal = nodal_dev; a.status = status_dev; a.iters = iters_dev;
    relmc_acc acc;                                        // the launch's partial records hold the island-rule count (of the units it did not list)
    Collected c;
    int rc = eval_collect(ctx, "relmc_mc_simulation", 1, a, 0, n, n_infeasible_out ? &acc : nullptr, c);
    if (rc) return rc;
    if (n_infeasible_out) *n_infeasible_out = acc.n_infeasible;
    RetryOut ro;
    rc = fail_retry(ctx, o, a.fail_threshold, nullptr, ro, &c.ms, c.known());
    if (rc) return rc;
    ctx->last_kernel_ms = c.ms;
    const size_t nb = (size_t)ctx->nb;
    for (size_t r = 0; r < ro.size(); ++r) {              // the second attempt's results in the place of the first's
        const RetryUnit u = ro[r];
        if (n_infeasible_out && u.island_rule) ++*n_infeasible_out;
        HIP_TRY(ctx, hipMemcpy(dns_dev + u.unit, &u.dns, sizeof(double), hipMemcpyHostToDevice));
        if (nodal_dev) HIP_TRY(ctx, hipMemcpy(nodal_dev + u.unit * nb, u.nodal, sizeof(double) * nb, hipMemcpyHostToDevice));
        if (status_dev) HIP_TRY(ctx, hipMemcpy(status_dev + u.unit, &u.status, sizeof(int32_t), hipMemcpyHostToDevice));
        if (iters_dev) HIP_TRY(ctx, hipMemcpy(iters_dev + u.unit, &u.iters, sizeof(int32_t), hipMemcpyHostToDevice));
    }
    return RELMC_OK;
}

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

int32_t relmc_mc_simulation_dev(relmc_ctx* ctx, const uint8_t* states_dev, int64_t n, const relmc_solver_opts* opts,
                                double* dns_dev, double* nodal_dev, int32_t* status_dev, int32_t* iters_dev)
{
    return mc_simulation_dev_impl(ctx, states_dev, n, opts, dns_dev, nodal_dev, status_dev, iters_dev, nullptr);
}

int32_t relmc_mc_simulation(relmc_ctx* ctx, const uint8_t* states_host, int64_t n, const relmc_solver_opts* opts,
                            double* dns_host, double* nodal_host, int32_t* status_host, int32_t* iters_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_case) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_mc_simulation: no case loaded");
    if (n < 0 || (n > 0 && (!states_host || !dns_host))) return fail(ctx, RELMC_ERR_INVALID, "relmc_mc_simulation: bad arguments");
    if (n == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return pipe_run(ctx, states_host, nullptr, n, solver_opts_or_default(opts), 1e-4 /* nsqMain.m:270 */, dns_host, nodal_host, status_host, iters_host);
}

int32_t relmc_nsq_accumulate(relmc_ctx* ctx, uint64_t seed, uint64_t first_index, int64_t n, const relmc_solver_opts* opts,
                             relmc_acc* acc_out)
{
    return nsq_accumulate_impl(ctx, seed, first_index, n, opts, acc_out, nullptr);
}

}  // extern "C"
