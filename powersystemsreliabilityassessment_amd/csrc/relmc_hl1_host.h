// relmc_hl1_host.h — host code the HL1 record models share: the unit and argument checks, the chunk rule, and the one loop that launches
// a model chunk by chunk and sums its year records (hl1_run_records), the checks and fills of the storage and weather-year tracks, and the
// one body of relmc_hl1_var_seq and relmc_hl1_stress_seq (hl1_weather_seq).
// Host only.  `who` is the calling function's name, for the message.
// The buffer pair of a model, Hl1Records, is in relmc_ctx.h: the context holds one per model by value.
#pragma once
#include <algorithm>
#include <cstring>

#include "relmc_ctx.h"

namespace relmc_host {

// relmc_hl1_seq_load and relmc_hl1_area_load (in relmc_seq.hip): the per-unit rule of the chronology models (capacity finite, MTTF and
// MTTR finite and positive); fills cap / mttf / mttr and q = mttr / (mttf + mttr)
int hl1_units_fill(relmc_ctx* ctx, const char* who, int ngen, const double* capacity_mw, const double* mttf_h, const double* mttr_h,
                   double* cap, double* mttf, double* mttr, double* q);
// what every call over n_chains chains of years_per_chain years checks first
inline bool hl1_chain_args_ok(const void* acc, int64_t n_chains, int32_t years_per_chain, int32_t start)
{
    return acc && n_chains >= 0 && years_per_chain >= 1 && (start == RELMC_HL1_START_ALL_UP || start == RELMC_HL1_START_STATIONARY);
}
// The chunk rule: items (chains; the planning model's years) of one launch, at least one, so that it holds at most budget_records records
// when an item counts records_per_item.  What an item counts is each model's own and part of its results: the launches order the sums.
constexpr int64_t kHl1RecordBudget = (int64_t)1 << 22;       // ~4M year records: 96 MB
inline int64_t hl1_chunk_items(int64_t n_items, int64_t budget_records, int64_t records_per_item)
{
    return std::max<int64_t>(1, std::min<int64_t>(n_items, budget_records / records_per_item));
}
inline int64_t hl1_reduce_blocks(int64_t n) { const int64_t b = (n + 255) / 256; return b < 1024 ? b : 1024; }   // workgroups over a slice of n records
// The tail of a launch, after the model kernel (in relmc_seq.hip): relmc_hl1_reduce_kernel over each of `rows` slices of n records
// (rec[row][n][3], fixed order) into dpart[row][blocks][6], ev1 behind the last reduction, then the copy of the partials to `part` queued
int hl1_reduce_queue(relmc_ctx* ctx, const char* who, const double* rec, int64_t n, int rows, double* dpart, std::vector<double>& part);
// After finish_timing: sum[row][6] += the partials, block by block (the order is part of the results)
inline void hl1_reduce_add(const std::vector<double>& part, int rows, double* sum)
{
    const size_t blocks = part.size() / 6 / (size_t)rows;
    for (int r = 0; r < rows; ++r)
        for (size_t b = 0; b < blocks; ++b)
            for (int j = 0; j < 6; ++j) sum[(size_t)r * 6 + j] += part[((size_t)r * blocks + b) * 6 + j];
}
inline void hl1_acc_fill(relmc_hl1_seq_acc* acc, int64_t years, const double* sum)
{
    acc->years = years;
    acc->sum_lole = sum[0]; acc->sum_eue = sum[1]; acc->sum_lolf = sum[2];
    acc->sum_lole2 = sum[3]; acc->sum_eue2 = sum[4]; acc->sum_lolf2 = sum[5];
}

// The launches of a record model: n_items items, `per` (hl1_chunk_items) to a launch, each with rec_per_item records in every one of the
// `slices` slices of R.years ([slice][record][3], packed for the launch's own record count; R grows to the largest launch).  sum[slice][6],
// zeroed by the caller, gets the fixed-order sums, ctx->last_kernel_ms the kernel time of all launches.  The model supplies, for the
// items [i0, i0 + ni) with nrec = ni * rec_per_item records: launch, which queues its kernel; copies -> code, which queues the copies
// to the host; after, the host's work on what they brought once the stream is synchronised.
template <class Launch, class Copies, class After>
int hl1_run_records(relmc_ctx* ctx, const char* who, Hl1Records& R, int64_t n_items, int64_t per, int64_t rec_per_item, int slices, double* sum,
                    Launch&& launch, Copies&& copies, After&& after)
{
    const int64_t rec_max = per * rec_per_item;
    HIP_TRY(ctx, R.years.grow((size_t)rec_max * 3 * slices));
    HIP_TRY(ctx, R.part.grow((size_t)hl1_reduce_blocks(rec_max) * 6 * slices));
    std::vector<double> part;
    double kernel_ms = 0.0;
    for (int64_t i0 = 0; i0 < n_items; i0 += per) {
        const int64_t ni = std::min(per, n_items - i0), nrec = ni * rec_per_item;
        (void)hipEventRecord(ctx->ev0, ctx->stream);
        launch(i0, ni, nrec);
        if (const int rc = hl1_reduce_queue(ctx, who, R.years.get(), nrec, slices, R.part.get(), part)) return rc;
        if (const int rc = copies(i0, ni, nrec)) return rc;
        if (finish_timing(ctx) != RELMC_OK) return fail(ctx, RELMC_ERR_HIP, std::string(who) + ": synchronisation failed");
        kernel_ms += ctx->last_kernel_ms;
        hl1_reduce_add(part, slices, sum);
        after(i0, ni, nrec);
    }
    ctx->last_kernel_ms = kernel_ms;
    return RELMC_OK;
}
inline void hl1_no_host_step(int64_t, int64_t, int64_t) {}   // `after` of a model whose copies land where they belong
// `after` of the area models: a launch's records stage[level][row][nrec][3], the first of them record first_rec of `total`, to
// years_host[level][total][rows]
inline void hl1_rows_to_host(const std::vector<double>& stage, int n_levels, int rows, int64_t nrec, int64_t total, int64_t first_rec, relmc_hl1_seq_year* years_host)
{
    for (int j = 0; j < n_levels; ++j)
        for (int64_t i = 0; i < nrec; ++i)
            for (int r = 0; r < rows; ++r) {
                relmc_hl1_seq_year& o = years_host[((size_t)j * total + (size_t)(first_rec + i)) * rows + r];
                const double* s = stage.data() + ((size_t)(j * rows + r) * nrec + i) * 3;
                o.lole = s[0]; o.eue = s[1]; o.lolf = s[2];
            }
}

// ---- what the storage and weather-year entry points check and fill alike: relmc_hl1_seq_storage, relmc_hl1_var_seq, relmc_hl1_stress_seq
// and relmc_hl1_area_var.  Here `who` is the message prefix "<function>: ".  Each entry point calls these in the order of its contract.

// n_storage in 0 .. RELMC_HL1_MAX_STORAGE, and an array to go with a positive count
inline int hl1_storage_count_check(relmc_ctx* ctx, const std::string& who, int32_t n_storage, const void* storage)
{
    if (n_storage < 0 || n_storage > RELMC_HL1_MAX_STORAGE)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_storage " + std::to_string(n_storage) + " not in 0.." + std::to_string(RELMC_HL1_MAX_STORAGE));
    if (n_storage > 0 && !storage) return fail(ctx, RELMC_ERR_INVALID, who + "n_storage > 0 without storage");
    return RELMC_OK;
}
// The field rule of one storage (include/relmc.h): every field finite, the powers and the energy not negative, the efficiencies in
// (0, 1], soc0_mwh in [0, energy_mwh].  st is the message prefix "<function>: storage <i>: ".
inline int hl1_storage_check(relmc_ctx* ctx, const std::string& st, const relmc_hl1_storage& v)
{
    const struct { const char* name; double x; } fields[6] = {{"charge_mw", v.charge_mw}, {"discharge_mw", v.discharge_mw}, {"energy_mwh", v.energy_mwh},
                                                               {"eta_charge", v.eta_charge}, {"eta_discharge", v.eta_discharge}, {"soc0_mwh", v.soc0_mwh}};
    for (const auto& f : fields)
        if (!std::isfinite(f.x)) return fail(ctx, RELMC_ERR_INVALID, st + f.name + " not finite");
    for (int q = 0; q < 3; ++q)
        if (fields[q].x < 0.0) return fail(ctx, RELMC_ERR_INVALID, st + fields[q].name + " is negative");
    for (int q = 3; q < 5; ++q)
        if (!(fields[q].x > 0.0 && fields[q].x <= 1.0)) return fail(ctx, RELMC_ERR_INVALID, st + fields[q].name + " not in (0, 1]");
    if (!(v.soc0_mwh >= 0.0 && v.soc0_mwh <= v.energy_mwh)) return fail(ctx, RELMC_ERR_INVALID, st + "soc0_mwh not in [0, energy_mwh]");
    return RELMC_OK;
}
// resource_scale[RELMC_HL1_VAR_MAX_RESOURCES] of the options against a library of n_res resources: finite, not negative, 0 beyond n_res;
// fills rscale[] (0.0 beyond n_res)
inline int hl1_resource_scales(relmc_ctx* ctx, const std::string& who, const double* resource_scale, int n_res, double* rscale)
{
    for (int r = 0; r < RELMC_HL1_VAR_MAX_RESOURCES; ++r) {
        const double s = resource_scale[r];
        const std::string rs = who + "resource_scale " + std::to_string(r);
        if (!std::isfinite(s)) return fail(ctx, RELMC_ERR_INVALID, rs + " not finite");
        if (s < 0.0) return fail(ctx, RELMC_ERR_INVALID, rs + " is negative");
        if (r >= n_res && s != 0.0) return fail(ctx, RELMC_ERR_INVALID, rs + " is not 0 with n_resources " + std::to_string(n_res));
        rscale[r] = r < n_res ? s : 0.0;
    }
    return RELMC_OK;
}
inline int hl1_pick_check(relmc_ctx* ctx, const std::string& who, int32_t pick, int32_t reserved)
{
    if (pick != RELMC_HL1_VAR_PICK_RANDOM && pick != RELMC_HL1_VAR_PICK_CYCLE)
        return fail(ctx, RELMC_ERR_INVALID, who + "pick " + std::to_string(pick) + " not 0 or 1");
    if (reserved != 0) return fail(ctx, RELMC_ERR_INVALID, who + "reserved is not 0");
    return RELMC_OK;
}
// weather_host[chain of the call][year] (nullptr: not wanted): the function the device works out (hl1_var_weather); the arguments are in range
inline void hl1_weather_fill(int32_t* weather_host, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t n_weather, int32_t pick)
{
    if (!weather_host) return;
    for (int64_t c = 0; c < n_chains; ++c)
        for (int32_t y = 0; y < years_per_chain; ++y)
            weather_host[c * years_per_chain + y] = relmc_hl1_var_weather_year(seed, first_chain + (uint64_t)c, y, years_per_chain, n_weather, pick);
}
// `copies` of the sequential storage-record models: the launch's two rows rec[row][nrec][3], the first record being record first_rec of the
// call, to the host arrays that were asked for
inline int hl1_two_row_copies(relmc_ctx* ctx, const double* rec, int64_t first_rec, int64_t nrec, relmc_hl1_seq_year* years_host,
                              relmc_hl1_storage_year* storage_years_host)
{
    if (years_host) HIP_TRY(ctx, hipMemcpyAsync(years_host + first_rec, rec, sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
    if (storage_years_host)
        HIP_TRY(ctx, hipMemcpyAsync(storage_years_host + first_rec, rec + (size_t)nrec * 3, sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
    return RELMC_OK;
}
// hl1_acc_fill's companion: s0 = the six sums of (lole, eue, lolf), s1 = those of (served_hours, discharged_mwh, charged_mwh)
inline void hl1_storage_acc_fill(relmc_hl1_storage_acc* acc, int64_t years, const double* s0, const double* s1)
{
    acc->years = years;
    acc->sum_lole = s0[0]; acc->sum_eue = s0[1]; acc->sum_lolf = s0[2]; acc->sum_lole2 = s0[3]; acc->sum_eue2 = s0[4]; acc->sum_lolf2 = s0[5];
    acc->sum_served = s1[0]; acc->sum_discharged = s1[1]; acc->sum_charged = s1[2];
    acc->sum_served2 = s1[3]; acc->sum_discharged2 = s1[4]; acc->sum_charged2 = s1[5];
}

// The body of relmc_hl1_var_seq (STRESS false: Args is Hl1VarArgs, the records go to hl1_var.rec) and of relmc_hl1_stress_seq (STRESS
// true: Hl1StressArgs, hl1_stress.rec), which adds the checks of its library against the fleet and the weather library and the fields of
// Args that hold it.  `name` is the entry point's, `kernel` its instantiation of relmc_hl1_storage_track_kernel.
template <bool STRESS, class Args, class Kernel>
int hl1_weather_seq(relmc_ctx* ctx, const char* name, Kernel kernel, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain,
                    int32_t start, const relmc_hl1_var_opts* opts, int32_t n_storage, const relmc_hl1_storage* storage, relmc_hl1_storage_acc* acc,
                    relmc_hl1_seq_year* years_host, relmc_hl1_storage_year* storage_years_host, int32_t* weather_host)
{
    const std::string who = std::string(name) + ": ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_seq_load has not been called");
    if (!ctx->has_hl1_var) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_var_load has not been called");
    if (STRESS && !ctx->has_hl1_stress) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_stress_load has not been called");
    auto& S = ctx->hl1_seq;
    auto& V = ctx->hl1_var;
    auto& X = ctx->hl1_stress;
    if (S.nhours != V.nhours)
        return fail(ctx, RELMC_ERR_INVALID, who + "nhours of relmc_hl1_seq_load " + std::to_string(S.nhours) + " is not nhours of relmc_hl1_var_load " + std::to_string(V.nhours));
    if constexpr (STRESS) {
        if (X.n_units != S.ngen)
            return fail(ctx, RELMC_ERR_INVALID, who + "n_units of relmc_hl1_stress_load " + std::to_string(X.n_units) + " is not the fleet's " + std::to_string(S.ngen));
        if (X.n_weather != V.n_weather)
            return fail(ctx, RELMC_ERR_INVALID, who + "n_weather of relmc_hl1_stress_load " + std::to_string(X.n_weather) + " is not n_weather of relmc_hl1_var_load " + std::to_string(V.n_weather));
        if (X.nhours != V.nhours)
            return fail(ctx, RELMC_ERR_INVALID, who + "nhours of relmc_hl1_stress_load " + std::to_string(X.nhours) + " is not nhours of relmc_hl1_var_load " + std::to_string(V.nhours));
    }
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (!opts) return fail(ctx, RELMC_ERR_INVALID, who + "opts is null");
    if (!std::isfinite(opts->scale) || !std::isfinite(opts->shift)) return fail(ctx, RELMC_ERR_INVALID, who + "scale / shift not finite");
    Args A; std::memset(&A, 0, sizeof(A));
    if (const int rc = hl1_resource_scales(ctx, who, opts->resource_scale, V.n_res, A.rscale)) return rc;
    if (const int rc = hl1_pick_check(ctx, who, opts->pick, opts->reserved)) return rc;
    if (const int rc = hl1_storage_count_check(ctx, who, n_storage, storage)) return rc;
    for (int i = 0; i < n_storage; ++i) {
        const relmc_hl1_storage& v = storage[i];
        const std::string st = who + "storage " + std::to_string(i) + ": ";
        if (const int rc = hl1_storage_check(ctx, st, v)) return rc;
        A.st[i] = v;
    }
    A.scale = opts->scale; A.shift = opts->shift; A.n_storage = n_storage;
    A.n_res = V.n_res; A.n_weather = V.n_weather; A.pick = opts->pick;
    A.out = V.out.get(); A.wload = V.has_load ? V.load.get() : nullptr;
    if constexpr (STRESS) { A.cum = X.cum.get(); A.ucls = X.ucls.get(); A.n_classes = X.n_classes; }
    std::memset(acc, 0, sizeof(*acc));
    if (n_chains == 0) return RELMC_OK;
    hl1_weather_fill(weather_host, seed, first_chain, n_chains, years_per_chain, V.n_weather, opts->pick);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    Hl1Records& R = STRESS ? X.rec : V.rec;
    double sum[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * 2);             // a chain counts its records of both rows
    const int rc = hl1_run_records(ctx, name, R, n_chains, per, years_per_chain, 2, sum,
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, A, R.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) { return hl1_two_row_copies(ctx, R.years.get(), c0 * years_per_chain, nrec, years_host, storage_years_host); },
        hl1_no_host_step);
    if (rc) return rc;
    hl1_storage_acc_fill(acc, n_chains * years_per_chain, sum, sum + 6);
    return RELMC_OK;
}

}  // namespace relmc_host
