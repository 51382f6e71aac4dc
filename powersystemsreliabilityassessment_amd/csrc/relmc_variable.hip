// relmc_variable.hip — weather-year wind and solar resources on the HL1 sequential chronology, with storage (relmc_hl1_var_load,
// relmc_hl1_var_seq, relmc_hl1_var_weather_year, contract in include/relmc.h): the fleet of relmc_hl1_seq_load (relmc_seq.hip) against a
// weather library in a slot of its own, with the storages of relmc_hl1_seq_storage given in the call.  A unit of its own, so that the
// code objects of relmc_seq.hip and relmc_storage.hip stay what they were; the kernel is the weather track of relmc_hl1_storage_kernels.h, the
// body of relmc_hl1_var_seq relmc_hl1_host.h's hl1_weather_seq, which relmc_hl1_stress_seq shares.  The two rows of year records, (lole, eue, lolf) and
// (served_hours, discharged_mwh, charged_mwh), are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_hl1_storage_kernels.h"

using namespace relmc_host;

static_assert(sizeof(relmc_hl1_var_opts) == 88, "relmc_hl1_var_opts is 88 bytes");

namespace {
// Philox4x32-10 on the host, word 0 only (relmc_devfn.h's philox4x32_10 in plain integer arithmetic)
uint32_t philox_word0(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1)
{
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
        c0 = n0; c1 = (uint32_t)p1; c2 = n2; c3 = (uint32_t)p0;
        k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
    }
    return c0;
}
// hl1_var_weather (relmc_hl1_storage_devfn.h) on the host; the arguments are in range
int32_t weather_year(uint64_t seed, uint64_t chain, int32_t y, int32_t years, int32_t n_weather, int32_t pick)
{
    if (pick == RELMC_HL1_VAR_PICK_CYCLE) return (int32_t)((chain * (uint64_t)years + (uint64_t)y) % (uint64_t)n_weather);
    const uint32_t x = philox_word0((uint32_t)chain, (uint32_t)(chain >> 32), RELMC_HL1_VAR_TAG, (uint32_t)y, (uint32_t)seed, (uint32_t)(seed >> 32));
    return (int32_t)(((uint64_t)x * (uint64_t)n_weather) >> 32);
}
}  // namespace

extern "C" {

int32_t relmc_hl1_var_weather_year(uint64_t seed, uint64_t chain, int32_t year, int32_t years_per_chain, int32_t n_weather, int32_t pick)
{
    if (year < 0 || years_per_chain < 1 || n_weather < 1 || n_weather > RELMC_HL1_VAR_MAX_WEATHER) return -1;
    if (pick != RELMC_HL1_VAR_PICK_RANDOM && pick != RELMC_HL1_VAR_PICK_CYCLE) return -1;
    return weather_year(seed, chain, year, years_per_chain, n_weather, pick);
}

int32_t relmc_hl1_var_load(relmc_ctx* ctx, int32_t n_weather, int32_t n_resources, int32_t nhours, const double* output_mw, const double* load_mw)
{
    const std::string who = "relmc_hl1_var_load: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (n_weather < 1 || n_weather > RELMC_HL1_VAR_MAX_WEATHER)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_weather " + std::to_string(n_weather) + " not in 1.." + std::to_string(RELMC_HL1_VAR_MAX_WEATHER));
    if (n_resources < 0 || n_resources > RELMC_HL1_VAR_MAX_RESOURCES)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_resources " + std::to_string(n_resources) + " not in 0.." + std::to_string(RELMC_HL1_VAR_MAX_RESOURCES));
    if (nhours < 1) return fail(ctx, RELMC_ERR_INVALID, who + "nhours " + std::to_string(nhours) + " is not positive");
    if (n_resources > 0 && !output_mw) return fail(ctx, RELMC_ERR_INVALID, who + "n_resources > 0 without output_mw");
    // the kernel indexes both tables in 32 bits
    if ((int64_t)n_weather * std::max<int64_t>(n_resources, 1) * nhours >= ((int64_t)1 << 31))
        return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "n_weather * max(n_resources, 1) * nhours is 2^31 or more");
    const size_t H = (size_t)nhours, n_out = (size_t)n_weather * (size_t)n_resources * H, n_load = (size_t)n_weather * H;
    for (size_t i = 0; i < n_out; ++i)
        if (!std::isfinite(output_mw[i]) || output_mw[i] < 0.0) {
            const std::string where = "output of weather year " + std::to_string(i / H / (size_t)n_resources) + ", resource " +
                                      std::to_string(i / H % (size_t)n_resources) + ", hour " + std::to_string(i % H);
            return fail(ctx, RELMC_ERR_INVALID, who + where + (std::isfinite(output_mw[i]) ? " is negative" : " not finite"));
        }
    if (load_mw)
        if (const int64_t bad = first_non_finite(load_mw, (int64_t)n_load); bad >= 0)
            return fail(ctx, RELMC_ERR_INVALID, who + "load of weather year " + std::to_string((size_t)bad / H) + ", hour " + std::to_string((size_t)bad % H) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& V = ctx->hl1_var;
    ctx->has_hl1_var = false;
    HIP_TRY(ctx, V.out.grow(std::max<size_t>(n_out, 1)));
    if (n_out) HIP_TRY(ctx, hipMemcpy(V.out.get(), output_mw, sizeof(double) * n_out, hipMemcpyHostToDevice));
    if (load_mw) {
        HIP_TRY(ctx, V.load.grow(n_load));
        HIP_TRY(ctx, hipMemcpy(V.load.get(), load_mw, sizeof(double) * n_load, hipMemcpyHostToDevice));
    }
    V.n_weather = n_weather; V.n_res = n_resources; V.nhours = nhours; V.has_load = load_mw != nullptr;
    ctx->has_hl1_var = true;
    return RELMC_OK;
}

int32_t relmc_hl1_var_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                          const relmc_hl1_var_opts* opts, int32_t n_storage, const relmc_hl1_storage* storage,
                          relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_storage_year* storage_years_host,
                          int32_t* weather_host)
{
    return hl1_weather_seq<false, Hl1VarArgs>(ctx, "relmc_hl1_var_seq", relmc_hl1_storage_track_kernel<HL1_TRACK_WEATHER>, seed, first_chain, n_chains, years_per_chain,
                                              start, opts, n_storage, storage, acc, years_host, storage_years_host, weather_host);
}

}  // extern "C"
