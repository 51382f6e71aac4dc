// relmc_plan.hip — the HL1 planning model's Monte Carlo: planned maintenance, energy-limited units and load forecast uncertainty
// (GeneratingAdequacy/generating_adequancy_comparative.jl:15-120, tail_risk.jl:12-91; contract in include/relmc.h).
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_plan_kernels.h"

using namespace relmc_host;

extern "C" {

int32_t relmc_hl1_plan_load(relmc_ctx* ctx, int32_t ngen, const double* capacity_mw, const double* for_rate,
                            const int32_t* outage_start_week, const int32_t* outage_weeks, const double* energy_limit_mwh,
                            int32_t nhours, const double* hourly_load_mw, double lfu_sigma_mw)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!capacity_mw || !for_rate || !outage_start_week || !outage_weeks || !energy_limit_mwh || !hourly_load_mw || ngen < 1 || nhours < 1 ||
        nhours >= (1 << 29) || !(std::isfinite(lfu_sigma_mw) && lfu_sigma_mw >= 0.0))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: bad arguments");
    if (ngen > NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_plan_load: more than 128 units");
    PlanCase P; std::memset(&P, 0, sizeof(P));
    P.ngen = ngen; P.nhours = nhours; P.nblk = (ngen + 5) / 4; P.sigma = lfu_sigma_mw;
    for (int e = 0; e < PLAN_MAX_ELU; ++e) P.elu_lim[e] = HUGE_VAL;
    for (int g = 0; g < ngen; ++g) {
        const std::string unit = " of unit " + std::to_string(g);
        if (!std::isfinite(capacity_mw[g])) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: capacity" + unit + " not finite");
        if (!(for_rate[g] >= 0.0 && for_rate[g] <= 1.0)) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: for_rate" + unit + " not in [0, 1]");
        if (outage_start_week[g] < 0 || outage_weeks[g] < 0)
            return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: negative maintenance week" + unit);
        if (std::isnan(energy_limit_mwh[g]) || energy_limit_mwh[g] < 0.0)
            return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: energy limit" + unit + " negative or NaN");
        PlanUnit& u = P.unit[g];
        double t = std::floor(for_rate[g] * 4294967296.0);
        if (!(t > 0)) t = 0;
        if (t > 4294967295.0) t = 4294967295.0;
        u.thr = (uint32_t)t; u.cap = capacity_mw[g]; u.slot = -1;
        if (outage_start_week[g] >= 1 && outage_weeks[g] >= 1) {               // weeks start .. start + weeks - 1 = hours [lo, hi) clipped to the year
            const int64_t lo = ((int64_t)outage_start_week[g] - 1) * 168, hi = lo + (int64_t)outage_weeks[g] * 168;
            u.mlo = (int32_t)std::min<int64_t>(lo, nhours); u.mhi = (int32_t)std::min<int64_t>(hi, nhours);
        }
        if (energy_limit_mwh[g] != HUGE_VAL) {
            if (P.n_elu == PLAN_MAX_ELU) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_plan_load: more than 8 energy-limited units");
            u.slot = P.n_elu; P.elu_cap[P.n_elu] = capacity_mw[g]; P.elu_lim[P.n_elu] = energy_limit_mwh[g]; ++P.n_elu;
        }
    }
    if (const int64_t bad = first_non_finite(hourly_load_mw, nhours); bad >= 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan_load: load of hour " + std::to_string(bad) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_plan;
    ctx->has_hl1_plan = false;
    HIP_TRY(ctx, S.dcase.grow(1));
    HIP_TRY(ctx, S.load.grow((size_t)nhours));
    HIP_TRY(ctx, hipMemcpy(S.dcase.get(), &P, sizeof(P), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.load.get(), hourly_load_mw, sizeof(double) * nhours, hipMemcpyHostToDevice));
    S.nhours = nhours; S.n_elu = P.n_elu; ctx->has_hl1_plan = true;
    return RELMC_OK;
}

int32_t relmc_hl1_plan(relmc_ctx* ctx, uint64_t seed, uint64_t first_year, int64_t n_years, relmc_hl1_seq_acc* acc,
                       relmc_hl1_seq_year* years_host, int64_t* hour_loss_count_host, double* elu_energy_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_plan) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_plan: relmc_hl1_plan_load has not been called");
    if (!acc || n_years < 0) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_plan: bad arguments");
    std::memset(acc, 0, sizeof(*acc));
    auto& S = ctx->hl1_plan;
    if (n_years == 0) {
        if (hour_loss_count_host) std::memset(hour_loss_count_host, 0, sizeof(int64_t) * S.nhours);
        return RELMC_OK;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    // years go in launches of at most 2^20 (24 MB of records, 64 MB of ELU energies); a year's records never depend on the launch it is in
    const int64_t per = hl1_chunk_items(n_years, (int64_t)1 << 20, 1);
    const bool want_elu = elu_energy_host && S.n_elu > 0;
    if (want_elu) HIP_TRY(ctx, S.elu.grow((size_t)per * S.n_elu));
    HIP_TRY(ctx, S.hours.grow((size_t)S.nhours));
    HIP_TRY(ctx, hipMemsetAsync(S.hours.get(), 0, sizeof(unsigned long long) * S.nhours, ctx->stream));
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int rc = hl1_run_records(ctx, "relmc_hl1_plan", S.rec, n_years, per, 1, 1, sum,
        [&](int64_t y0, int64_t ny, int64_t) {
            hipLaunchKernelGGL(relmc_hl1_plan_kernel, dim3((unsigned)((ny + 255) / 256)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_year + (uint64_t)y0, ny, S.rec.years.get(), want_elu ? S.elu.get() : nullptr, S.hours.get());
        },
        [&](int64_t y0, int64_t ny, int64_t) -> int {
            if (years_host)
                HIP_TRY(ctx, hipMemcpyAsync(years_host + y0, S.rec.years.get(), sizeof(double) * 3 * ny, hipMemcpyDeviceToHost, ctx->stream));
            if (want_elu)
                HIP_TRY(ctx, hipMemcpyAsync(elu_energy_host + y0 * S.n_elu, S.elu.get(), sizeof(double) * S.n_elu * ny, hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        hl1_no_host_step);
    if (rc) return rc;
    if (hour_loss_count_host) {
        static_assert(sizeof(unsigned long long) == sizeof(int64_t), "hour counts are 64-bit");
        HIP_TRY(ctx, hipMemcpy(hour_loss_count_host, S.hours.get(), sizeof(int64_t) * S.nhours, hipMemcpyDeviceToHost));
    }
    hl1_acc_fill(acc, n_years, sum);
    return RELMC_OK;
}

}  // extern "C"
