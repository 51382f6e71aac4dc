// relmc_stress.hip — weather-dependent forced outage rates on the HL1 sequential chronology (relmc_hl1_stress_load, relmc_hl1_stress_seq,
// relmc_hl1_stress_cumulative, relmc_hl1_stress_failure_time, contract in include/relmc.h): the fleet of relmc_hl1_seq_load against the
// weather library of relmc_hl1_var_load, with a failure-rate multiplier per weather year, outage class and hour in a slot of its own.
// A unit of its own, so that the code objects of relmc_seq.hip, relmc_storage.hip and relmc_variable.hip stay what they were; the kernel is
// the stress track of relmc_hl1_storage_kernels.h, the body of relmc_hl1_stress_seq relmc_hl1_host.h's hl1_weather_seq.  The two
// rows of year records are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_hl1_storage_kernels.h"

using namespace relmc_host;

namespace {
// G[0] = 0, G[j + 1] = G[j] + m[j]: one rounded addition per hour
void cumulative(int32_t nhours, const double* m, double* G)
{
    G[0] = 0.0;
    for (int32_t j = 0; j < nhours; ++j) G[j + 1] = G[j] + m[j];
}
}  // namespace

extern "C" {

int32_t relmc_hl1_stress_cumulative(int32_t nhours, const double* fail_mult_row, double* cum_out)
{
    if (nhours < 1 || !fail_mult_row || !cum_out) return RELMC_ERR_INVALID;
    for (int32_t j = 0; j < nhours; ++j)
        if (!std::isfinite(fail_mult_row[j]) || fail_mult_row[j] < 0.0) return RELMC_ERR_INVALID;
    cumulative(nhours, fail_mult_row, cum_out);
    return RELMC_OK;
}

double relmc_hl1_stress_failure_time(double t, double e, int32_t nhours, int32_t years_per_chain, const int32_t* weather, const double* cum)
{
    const double nan = std::numeric_limits<double>::quiet_NaN();
    if (!(t >= 0.0) || !(e >= 0.0) || !std::isfinite(t) || nhours < 1 || years_per_chain < 1 || !weather || !cum) return nan;
    for (int32_t y = 0; y < years_per_chain; ++y)
        if (weather[y] < 0 || weather[y] >= RELMC_HL1_VAR_MAX_WEATHER) return nan;
    return relmc::hl1_stress_failure_time(t, e, nhours, years_per_chain, [&](int y) { return cum + (size_t)weather[y] * ((size_t)nhours + 1); });
}

int32_t relmc_hl1_stress_load(relmc_ctx* ctx, int32_t n_weather, int32_t n_classes, int32_t nhours, const double* fail_mult, int32_t n_units,
                              const int32_t* unit_class)
{
    const std::string who = "relmc_hl1_stress_load: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (n_weather < 1 || n_weather > RELMC_HL1_VAR_MAX_WEATHER)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_weather " + std::to_string(n_weather) + " not in 1.." + std::to_string(RELMC_HL1_VAR_MAX_WEATHER));
    if (n_classes < 1 || n_classes > RELMC_HL1_STRESS_MAX_CLASSES)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_classes " + std::to_string(n_classes) + " not in 1.." + std::to_string(RELMC_HL1_STRESS_MAX_CLASSES));
    if (nhours < 1) return fail(ctx, RELMC_ERR_INVALID, who + "nhours " + std::to_string(nhours) + " is not positive");
    if (n_units < 1 || n_units > relmc::NCOMPMAX)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_units " + std::to_string(n_units) + " not in 1.." + std::to_string(relmc::NCOMPMAX));
    if (!fail_mult || !unit_class) return fail(ctx, RELMC_ERR_INVALID, who + "fail_mult or unit_class is null");
    // the kernel indexes the cumulative tables in 32 bits
    if ((int64_t)n_weather * n_classes * ((int64_t)nhours + 1) >= ((int64_t)1 << 31))
        return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "n_weather * n_classes * (nhours + 1) is 2^31 or more");
    const size_t H = (size_t)nhours, rows = (size_t)n_weather * (size_t)n_classes;
    for (size_t i = 0; i < rows * H; ++i)
        if (!std::isfinite(fail_mult[i]) || fail_mult[i] < 0.0) {
            const std::string where = "multiplier of weather year " + std::to_string(i / H / (size_t)n_classes) + ", class " +
                                      std::to_string(i / H % (size_t)n_classes) + ", hour " + std::to_string(i % H);
            return fail(ctx, RELMC_ERR_INVALID, who + where + (std::isfinite(fail_mult[i]) ? " is negative" : " not finite"));
        }
    for (int32_t k = 0; k < n_units; ++k)
        if (unit_class[k] < -1 || unit_class[k] >= n_classes)
            return fail(ctx, RELMC_ERR_INVALID, who + "class " + std::to_string(unit_class[k]) + " of unit " + std::to_string(k) + " not in -1.." + std::to_string(n_classes - 1));
    std::vector<double> G(rows * (H + 1));
    for (size_t r = 0; r < rows; ++r) cumulative(nhours, fail_mult + r * H, G.data() + r * (H + 1));
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& X = ctx->hl1_stress;
    ctx->has_hl1_stress = false;
    HIP_TRY(ctx, X.cum.grow(G.size()));
    HIP_TRY(ctx, hipMemcpy(X.cum.get(), G.data(), sizeof(double) * G.size(), hipMemcpyHostToDevice));
    HIP_TRY(ctx, X.ucls.grow((size_t)n_units));
    HIP_TRY(ctx, hipMemcpy(X.ucls.get(), unit_class, sizeof(int32_t) * (size_t)n_units, hipMemcpyHostToDevice));
    X.n_weather = n_weather; X.n_classes = n_classes; X.nhours = nhours; X.n_units = n_units;
    ctx->has_hl1_stress = true;
    return RELMC_OK;
}

int32_t relmc_hl1_stress_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                             const relmc_hl1_var_opts* opts, int32_t n_storage, const relmc_hl1_storage* storage,
                             relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_storage_year* storage_years_host,
                             int32_t* weather_host)
{
    return hl1_weather_seq<true, relmc::Hl1StressArgs>(ctx, "relmc_hl1_stress_seq", relmc::relmc_hl1_storage_track_kernel<relmc::HL1_TRACK_STRESS>, seed, first_chain, n_chains,
                                                       years_per_chain, start, opts, n_storage, storage, acc, years_host, storage_years_host, weather_host);
}

}  // extern "C"
