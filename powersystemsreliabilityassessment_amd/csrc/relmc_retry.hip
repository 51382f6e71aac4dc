// relmc_retry.hip — second chances for the units the primary static elimination order does not converge on: the kernel's list of such
// units, their re-evaluation under further static orders and, last, under a dense partially pivoted solve (what MATLAB's `\` does under
// MIPS, mc_simulation.m:41).  DESIGN.md 6.3.
#include <algorithm>
#include <cstring>

#include "relmc_ctx.h"

namespace relmc_host {

// ---- second chance for the units the primary elimination order does not converge on ---------------------------------------------
// The block elimination runs in an order fixed per case; on a few states (6.7e-7 of the RTS-96 scenarios, 4e-10 on RTS-24) that order
// meets a stiff line next to a bus with an interior injection and the Newton steps of the last iterations lose their digits (DESIGN.md
// 6.3).  Which states depends on the order: of the 67 such RTS-96 states in 1e8 samples, 66 converge under the same elimination rule with
// the ties broken the other way (same pass counts).  The kernel lists the units it ends non-converged instead of accumulating them; they
// are evaluated again here under that second order and their results take the place of the first attempt's.
// List capacity: 4096 + 1/256 of the units of the call.  relmc_case_load's calibration leaves a primary order in place only if it fails on
// at most 0.1 % of a probe sample, so a list of 0.39 % + 4096 entries does not overflow on a calibrated case; if it does anyway the fused
// path grows the list and evaluates the chunk again (the launch is deterministic), the other paths count the units that kept their
// first-attempt results in relmc_retry_overflow.
uint32_t fail_cap_for(int64_t call_units)
{
    // steady-state size: 4096 + 1/256 of the call's units, at most 2^20 entries (48 MB; a 1e9-sample call used to hold 190 MB for a list that a
    // calibrated case fills to a few hundred entries).  The fused path grows the list up to kFailCapMax and re-runs the chunk if it overflows.
    const int64_t c = (int64_t)kFailCapMin + call_units / 256;
    return c > (int64_t)kFailCapSteady ? kFailCapSteady : (uint32_t)c;
}
int fail_count_ensure(relmc_ctx* ctx)
{
    auto& R = ctx->retry;
    if (!R.fail_count.get()) {
        HIP_TRY(ctx, R.fail_count.grow(R.kCountWords));
        HIP_TRY(ctx, hipMemsetAsync(R.fail_count.get(), 0, R.kCountBytes, ctx->stream));
    }
    return RELMC_OK;
}
int fail_list_ensure(relmc_ctx* ctx, uint32_t cap)
{
    auto& R = ctx->retry;
    { const int rc = fail_count_ensure(ctx); if (rc) return rc; }
    if (cap <= R.fail.size()) return RELMC_OK;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));      // the list is dropped below: no launch may still write to it
    HIP_TRY(ctx, R.fail.grow(cap));
    return RELMC_OK;
}

int alt_ensure(relmc_ctx* ctx, int v)          // v = 0, 1: which further order
{
    if (ctx->alt_state[v]) return ctx->alt_state[v] > 0 ? RELMC_OK : RELMC_ERR_UNSUPPORTED;
    ctx->alt_state[v] = -1;
    if (!ctx->case_copy.valid) return RELMC_ERR_UNSUPPORTED;
    const std::string keep = ctx->err;
    const int rc = case_load_image(ctx, &ctx->case_copy.d, v + 1);
    ctx->err = keep;                               // a case whose further order does not fit simply has one attempt less
    if (rc == RELMC_OK) ctx->alt_state[v] = 1;
    return rc;
}

// arms the kernel's list for the next launch(es); `reset` zeroes the count (first launch of a call) and sizes the list for the
// `call_units` units all launches of the call evaluate together
int fail_arm(relmc_ctx* ctx, EvalArgs& a, int64_t unit_base, bool reset, int64_t call_units)
{
    a.fail_list = nullptr; a.fail_count = nullptr; a.fail_cap = 0; a.unit_base = unit_base;
    if (ctx->sw.no_retry) return RELMC_OK;      // diagnosis switch: the first attempt's results as they are
    // (a case whose further static orders do not fit the tile is armed all the same: the dense pivoted level needs no second image)
    if (reset || !ctx->retry.fail.get()) {
        const int rc = fail_list_ensure(ctx, fail_cap_for(call_units));
        if (rc) return rc;
    }
    // the count is zero whenever a call has collected its list (fail_retry zeroes it after a non-empty one), so the common case costs no
    // memset launch; only a call that was abandoned between arming and collecting leaves it to be cleared here
    if (reset && ctx->retry.fail_dirty) { HIP_TRY(ctx, hipMemsetAsync(ctx->retry.fail_count.get(), 0, ctx->retry.kCountBytes, ctx->stream)); }
    if (reset) ctx->retry.fail_dirty = true;
    a.fail_list = ctx->retry.fail.get(); a.fail_count = ctx->retry.fail_count.get(); a.fail_cap = (uint32_t)ctx->retry.fail.size();
    return RELMC_OK;
}

int eval_collect(relmc_ctx* ctx, const char* who, int mode, EvalArgs& a, int64_t unit_base, int64_t call_units, relmc_acc* acc, Collected& c)
{
    int rows = 0;
    int rc = fail_arm(ctx, a, unit_base, true, call_units);
    if (rc == RELMC_OK) rc = launch_eval(ctx, mode, a, &rows);
    if (rc == RELMC_OK && acc) rc = launch_finalize(ctx, rows);
    if (rc) return rc;
    // accumulators and the count of listed units come back in ONE synchronisation, through the context's pinned staging words (two more
    // blocking 4-byte copies per launch used to follow the kernel)
    auto* const st = ctx->hstage.get();
    c.armed = a.fail_count != nullptr;
    if ((acc && hipMemcpyAsync(&st->acc, ctx->dacc.get(), sizeof(relmc_acc), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess) ||
        (c.armed && hipMemcpyAsync(&st->fail_cnt, a.fail_count, sizeof(uint32_t), hipMemcpyDeviceToHost, ctx->stream) != hipSuccess))
        return fail(ctx, RELMC_ERR_HIP, std::string(who) + ": queueing the copy of the launch's results failed");
    rc = finish_timing(ctx);
    if (rc) return rc;
    if (acc) *acc = st->acc;
    c.listed = c.armed ? st->fail_cnt : 0u;
    c.ms = ctx->last_kernel_ms;
    return RELMC_OK;
}

// After the launches of a call have completed: the listed units (ascending), evaluated under the second order.  `scale` (optional) maps a
// unit to its load scale factor.  out.rec is empty when nothing was listed.  Adds the retry kernel's time to *ms.
int fail_retry(relmc_ctx* ctx, const relmc_solver_opts& o, double fail_threshold, const ScaleFn* scale_fn, RetryOut& out, double* ms, const uint32_t* known_count)
{
    const bool have_scale = scale_fn != nullptr;
    auto scale = [&](unsigned long long u) { return (*scale_fn)(u); };
    out.rec.clear();
    if (!ctx->retry.fail_count.get()) return RELMC_OK;
    uint32_t cnt = 0;
    if (known_count) cnt = *known_count;            // the caller read the count with its results (one synchronisation)
    else HIP_TRY(ctx, hipMemcpy(&cnt, ctx->retry.fail_count.get(), sizeof(cnt), hipMemcpyDeviceToHost));
    ctx->retry.fail_dirty = false;
    if (cnt == 0) return RELMC_OK;
    HIP_TRY(ctx, hipMemset(ctx->retry.fail_count.get(), 0, ctx->retry.kCountBytes));
    const uint32_t cap = (uint32_t)ctx->retry.fail.size();
    if (cnt > cap) {                                         // the units beyond the list were accumulated by the kernel as they were
        ctx->retry_overflow += (int64_t)(cnt - cap);
        cnt = cap;
    }
    out.rec.resize(cnt);
    HIP_TRY(ctx, hipMemcpy(out.rec.data(), ctx->retry.fail.get(), sizeof(FailRec) * cnt, hipMemcpyDeviceToHost));
    std::sort(out.rec.begin(), out.rec.end(), [](const FailRec& x, const FailRec& y) { return x.unit < y.unit; });
    const int ow = ctx->tile == 0 ? Tile24::OW : Tile96::OW;
    const size_t nb = (size_t)ctx->nb;
    auto& R = ctx->retry;
    // scratch rows of the re-evaluation, sized by what was listed (twice: the third order's compact rows); the bus count is the case's (reset by relmc_case_load)
    if ((int64_t)cnt > R.rows) { R.rows = kFailCapMin; while (R.rows < (int64_t)cnt) R.rows *= 2; }
    const size_t rc2 = (size_t)R.rows;
    HIP_TRY(ctx, R.keys.grow(rc2 * 2 * 8));
    HIP_TRY(ctx, R.dns.grow(rc2 * 2));
    HIP_TRY(ctx, R.meta.grow(rc2 * 2));
    HIP_TRY(ctx, R.nodal.grow(rc2 * 2 * nb));
    HIP_TRY(ctx, R.scale.grow(rc2 * 2));
    out.dns.resize(cnt); out.meta.resize(cnt); out.nodal.resize((size_t)cnt * nb); out.nb = nb;
    // first the whole list under the second order, then whatever is still non-converged under the third (the sets of states the three
    // orders fail on were disjoint on the 67 RTS-96 states of the fixture).  A case without further orders (they do not fit the tile)
    // repeats the primary one, so that the callers' bookkeeping is one path.
    const bool dense_first = ctx->sw.retry_dense_first;      // tests: the listed units straight to the dense pivoted solve
    auto converged = [](int32_t meta) { return (meta & 3) == 0 || (meta & 3) == 3; };
    // A level evaluates the list rows idx at the scratch row `base`.  The first level that runs: every row, in place (base 0).  A later one: the
    // rows still at status 1 or 2, compacted behind the list's rows and evaluated in ONE launch (round 2 launched once per unit), the results
    // copied over the rows they belong to.
    std::vector<uint32_t> idx(cnt), keys; std::vector<double> sc;
    for (uint32_t r = 0; r < cnt; ++r) idx[r] = r;
    size_t base = 0;
    // level 0, 1: the further static orders; level 2: the dense, partially pivoted solve (what MATLAB's `\` does under mips) for whatever
    // no static order converged on
    for (int level = dense_first ? relmc_ctx::kAlt : 0; level <= relmc_ctx::kAlt; ++level) {
        const bool dense = level == relmc_ctx::kAlt;
        const bool have = dense || alt_ensure(ctx, level) == RELMC_OK;
        if (level > 0 && !have) continue;
        if (base) {
            idx.clear();
            for (uint32_t r = 0; r < cnt; ++r) if (!converged(out.meta[r])) idx.push_back(r);
            if (idx.empty()) break;
        }
        const size_t m = idx.size();
        keys.resize(m * ow); sc.resize(m);
        for (size_t q = 0; q < m; ++q) { for (int w = 0; w < ow; ++w) keys[q * ow + w] = out.rec[idx[q]].mask[w]; if (have_scale) sc[q] = scale(out.rec[idx[q]].unit); }
        HIP_TRY(ctx, hipMemcpy(R.keys.get() + base * ow, keys.data(), sizeof(uint32_t) * keys.size(), hipMemcpyHostToDevice));
        if (have_scale) HIP_TRY(ctx, hipMemcpy(R.scale.get() + base, sc.data(), sizeof(double) * m, hipMemcpyHostToDevice));
        EvalArgs a = make_args(o);
        a.fail_threshold = fail_threshold;
        a.n = (int64_t)m; a.memo_keys = R.keys.get(); a.db_first = (int64_t)base; a.dns = R.dns.get(); a.status = R.meta.get(); a.nodal = R.nodal.get();
        a.load_scale = have_scale ? R.scale.get() + base : nullptr;
        int rows = 0;
        int rc = dense ? launch_eval(ctx, 6, a, &rows) : launch_eval(ctx, 4, a, &rows, nullptr, nullptr, have ? level + 1 : 0);
        if (rc) return rc;
        const double before = ctx->last_kernel_ms;
        rc = finish_timing(ctx);
        if (rc) return rc;
        if (ms) *ms += ctx->last_kernel_ms;
        ctx->last_kernel_ms = before;
        if (base) {
            for (size_t q = 0; q < m; ++q) {
                HIP_TRY(ctx, hipMemcpyAsync(R.dns.get() + idx[q], R.dns.get() + base + q, sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(R.meta.get() + idx[q], R.meta.get() + base + q, sizeof(int32_t), hipMemcpyDeviceToDevice, ctx->stream));
                HIP_TRY(ctx, hipMemcpyAsync(R.nodal.get() + (size_t)idx[q] * nb, R.nodal.get() + (base + q) * nb, sizeof(double) * nb, hipMemcpyDeviceToDevice, ctx->stream));
            }
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        }
        HIP_TRY(ctx, hipMemcpy(out.meta.data(), R.meta.get(), sizeof(int32_t) * cnt, hipMemcpyDeviceToHost));      // what is still left, for the next level
        if (dense) {
            ctx->retry_dense_units += (int64_t)m;
            for (size_t q = 0; q < m; ++q) if (converged(out.meta[idx[q]])) ctx->retry_dense_converged += 1;
        }
        base = (size_t)R.rows;
    }
    HIP_TRY(ctx, hipMemcpy(out.dns.data(), ctx->retry.dns.get(), sizeof(double) * cnt, hipMemcpyDeviceToHost));
    HIP_TRY(ctx, hipMemcpy(out.nodal.data(), ctx->retry.nodal.get(), sizeof(double) * cnt * nb, hipMemcpyDeviceToHost));
    ctx->retry_units += cnt;
    for (uint32_t r = 0; r < cnt; ++r) if (converged(out.meta[r])) ctx->retry_converged += 1;
    return RELMC_OK;
}

// the accumulators of one unit (what the kernel's output section adds for it), count-weighted
void acc_add_unit(relmc_acc* acc, const RetryUnit& u, int nb, int ncomp, double fail_threshold)
{
    const long long w = u.weight;
    const bool fail = u.dns > fail_threshold;
    acc->n += w;
    if (fail) acc->n_fail += w;
    if (u.status == 3) acc->n_singular += w;
    if (u.status == 1 || u.status == 2) acc->n_nonconverged += w;
    if (u.island_rule) acc->n_infeasible += w;
    acc->sum_iters += (long long)u.iters * w;
    if (u.dns != 0.0) { acc->sum_dns += (double)w * u.dns; acc->sum_dns2 += (double)w * u.dns * u.dns; }
    if (fail) for (int k = 0; k < ncomp; ++k) if ((u.mask[k >> 5] >> (k & 31)) & 1u) acc->comp_fail[k] += w;
    for (int i = 0; i < nb; ++i) acc->sum_nodal[i] += (double)w * u.nodal[i];
}

}  // namespace relmc_host

using namespace relmc_host;

extern "C" {

int32_t relmc_retry_stats(const relmc_ctx* ctx, int64_t* units_out, int64_t* converged_out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (units_out) *units_out = ctx->retry_units;
    if (converged_out) *converged_out = ctx->retry_converged;
    return RELMC_OK;
}

int32_t relmc_retry_overflow(const relmc_ctx* ctx, int64_t* units_out)
{
    if (!ctx || !units_out) return RELMC_ERR_INVALID;
    *units_out = ctx->retry_overflow;
    return RELMC_OK;
}

// units that went to the dense pivoted last resort since the case was loaded, and how many of them it converged on
int32_t relmc_retry_dense_stats(const relmc_ctx* ctx, int64_t* units_out, int64_t* converged_out)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (units_out) *units_out = ctx->retry_dense_units;
    if (converged_out) *converged_out = ctx->retry_dense_converged;
    return RELMC_OK;
}

}  // extern "C"
