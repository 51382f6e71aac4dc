// relmc_storage.hip — energy storage with a state of charge on the HL1 sequential chronology (relmc_hl1_seq_storage, contract in
// include/relmc.h): the model of relmc_hl1_seq_load (relmc_seq.hip) at one load level, with up to RELMC_HL1_MAX_STORAGE storages given in
// the call.  A unit of its own, so that relmc_seq.hip's code object stays what it was.  The two rows of year records, (lole, eue, lolf)
// and (served_hours, discharged_mwh, charged_mwh), are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_storage_kernels.h"

using namespace relmc_host;

static_assert(sizeof(relmc_hl1_storage) == 48, "relmc_hl1_storage is 48 bytes");
static_assert(sizeof(relmc_hl1_storage_year) == sizeof(relmc_hl1_seq_year), "both record rows are three doubles");
static_assert(sizeof(relmc_hl1_storage_acc) == 8 + 12 * sizeof(double), "relmc_hl1_storage_acc: years and the two rows' six sums");

extern "C" {

int32_t relmc_hl1_seq_storage(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                              double scale, double shift, int32_t n_storage, const relmc_hl1_storage* storage,
                              relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_storage_year* storage_years_host)
{
    const std::string who = "relmc_hl1_seq_storage: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_seq_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (!std::isfinite(scale) || !std::isfinite(shift)) return fail(ctx, RELMC_ERR_INVALID, who + "scale / shift not finite");
    if (n_storage < 0 || n_storage > RELMC_HL1_MAX_STORAGE)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_storage " + std::to_string(n_storage) + " not in 0.." + std::to_string(RELMC_HL1_MAX_STORAGE));
    if (n_storage > 0 && !storage) return fail(ctx, RELMC_ERR_INVALID, who + "n_storage > 0 without storage");
    Hl1StorageArgs A; std::memset(&A, 0, sizeof(A));
    A.scale = scale; A.shift = shift; A.n_storage = n_storage;
    for (int i = 0; i < n_storage; ++i) {
        const relmc_hl1_storage& v = storage[i];
        const std::string st = who + "storage " + std::to_string(i) + ": ";
        const struct { const char* name; double x; } fields[6] = {{"charge_mw", v.charge_mw}, {"discharge_mw", v.discharge_mw}, {"energy_mwh", v.energy_mwh},
                                                                   {"eta_charge", v.eta_charge}, {"eta_discharge", v.eta_discharge}, {"soc0_mwh", v.soc0_mwh}};
        for (const auto& f : fields)
            if (!std::isfinite(f.x)) return fail(ctx, RELMC_ERR_INVALID, st + f.name + " not finite");
        for (int q = 0; q < 3; ++q)
            if (fields[q].x < 0.0) return fail(ctx, RELMC_ERR_INVALID, st + fields[q].name + " is negative");
        for (int q = 3; q < 5; ++q)
            if (!(fields[q].x > 0.0 && fields[q].x <= 1.0)) return fail(ctx, RELMC_ERR_INVALID, st + fields[q].name + " not in (0, 1]");
        if (!(v.soc0_mwh >= 0.0 && v.soc0_mwh <= v.energy_mwh)) return fail(ctx, RELMC_ERR_INVALID, st + "soc0_mwh not in [0, energy_mwh]");
        A.st[i] = v;
    }
    std::memset(acc, 0, sizeof(*acc));
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_seq;
    auto& X = ctx->hl1_storage;
    double sum[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * 2);             // a chain counts its records of both rows
    const int rc = hl1_run_records(ctx, "relmc_hl1_seq_storage", X, n_chains, per, years_per_chain, 2, sum,
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(relmc_hl1_storage_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, A, X.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) -> int {
            if (years_host)
                HIP_TRY(ctx, hipMemcpyAsync(years_host + c0 * years_per_chain, X.years.get(), sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            if (storage_years_host)
                HIP_TRY(ctx, hipMemcpyAsync(storage_years_host + c0 * years_per_chain, X.years.get() + (size_t)nrec * 3, sizeof(double) * 3 * nrec,
                                            hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        hl1_no_host_step);
    if (rc) return rc;
    acc->years = n_chains * years_per_chain;
    acc->sum_lole = sum[0]; acc->sum_eue = sum[1]; acc->sum_lolf = sum[2]; acc->sum_lole2 = sum[3]; acc->sum_eue2 = sum[4]; acc->sum_lolf2 = sum[5];
    acc->sum_served = sum[6]; acc->sum_discharged = sum[7]; acc->sum_charged = sum[8];
    acc->sum_served2 = sum[9]; acc->sum_discharged2 = sum[10]; acc->sum_charged2 = sum[11];
    return RELMC_OK;
}

}  // extern "C"
