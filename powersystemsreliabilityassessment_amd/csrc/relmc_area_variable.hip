// relmc_area_variable.hip — weather-year resources and storages in the areas of the HL1 multi-area chronology (relmc_hl1_area_var_load,
// relmc_hl1_area_var, contract in include/relmc.h): the areas, units and ties of relmc_hl1_area_load (relmc_area.hip), with
// relmc_hl1_area_tie_outages' data when set, against a weather library in a slot of its own; the storages are given in the call.  A unit
// of its own, so that the code objects of relmc_area.hip and relmc_variable.hip stay what they were; the resource-scale, pick and
// per-storage checks, the weather_host fill and the accumulator fill are relmc_hl1_host.h's, shared with relmc_hl1_var_seq.  The two records of every row,
// (lole, eue, lolf) and (served_hours, discharged_mwh, charged_mwh), are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue,
// relmc_seq.hip), one slice at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_area_kernels.h"

using namespace relmc_host;

static_assert(sizeof(relmc_hl1_area_var_opts) == 208, "relmc_hl1_area_var_opts is 208 bytes");
static_assert(sizeof(relmc_hl1_area_storage) == 56, "relmc_hl1_area_storage is 56 bytes");
static_assert(sizeof(relmc::AreaVarArgs) < 4096, "AreaVarArgs must fit the kernel argument segment");

extern "C" {

int32_t relmc_hl1_area_var_load(relmc_ctx* ctx, int32_t n_areas, int32_t n_weather, int32_t n_resources, const int32_t* resource_area,
                                int32_t nhours, const double* output_mw, const double* load_mw)
{
    const std::string who = "relmc_hl1_area_var_load: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (n_areas < 1) return fail(ctx, RELMC_ERR_INVALID, who + "n_areas " + std::to_string(n_areas) + " is not positive");
    if (n_areas > RELMC_AREA_MAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "more than 8 areas");
    if (n_weather < 1 || n_weather > RELMC_HL1_VAR_MAX_WEATHER)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_weather " + std::to_string(n_weather) + " not in 1.." + std::to_string(RELMC_HL1_VAR_MAX_WEATHER));
    if (n_resources < 0 || n_resources > RELMC_HL1_VAR_MAX_RESOURCES)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_resources " + std::to_string(n_resources) + " not in 0.." + std::to_string(RELMC_HL1_VAR_MAX_RESOURCES));
    if (nhours < 1) return fail(ctx, RELMC_ERR_INVALID, who + "nhours " + std::to_string(nhours) + " is not positive");
    if (n_resources > 0 && !resource_area) return fail(ctx, RELMC_ERR_INVALID, who + "n_resources > 0 without resource_area");
    if (n_resources > 0 && !output_mw) return fail(ctx, RELMC_ERR_INVALID, who + "n_resources > 0 without output_mw");
    for (int r = 0; r < n_resources; ++r)
        if (resource_area[r] < 0 || resource_area[r] >= n_areas)
            return fail(ctx, RELMC_ERR_INVALID, who + "resource " + std::to_string(r) + " is in area " + std::to_string(resource_area[r]) + ", not in 0.." +
                                                std::to_string(n_areas - 1));
    // the kernel indexes both tables in 32 bits
    if ((int64_t)n_weather * std::max<int64_t>(std::max(n_resources, n_areas), 1) * nhours >= ((int64_t)1 << 31))
        return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "n_weather * max(n_resources, n_areas, 1) * nhours is 2^31 or more");
    const size_t H = (size_t)nhours, n_out = (size_t)n_weather * (size_t)n_resources * H, n_load = (size_t)n_weather * (size_t)n_areas * H;
    for (size_t i = 0; i < n_out; ++i)
        if (!std::isfinite(output_mw[i]) || output_mw[i] < 0.0) {
            const std::string where = "output of weather year " + std::to_string(i / H / (size_t)n_resources) + ", resource " +
                                      std::to_string(i / H % (size_t)n_resources) + ", hour " + std::to_string(i % H);
            return fail(ctx, RELMC_ERR_INVALID, who + where + (std::isfinite(output_mw[i]) ? " is negative" : " not finite"));
        }
    if (load_mw)
        if (const int64_t bad = first_non_finite(load_mw, (int64_t)n_load); bad >= 0)
            return fail(ctx, RELMC_ERR_INVALID, who + "load of weather year " + std::to_string((size_t)bad / H / (size_t)n_areas) + ", area " +
                                                std::to_string((size_t)bad / H % (size_t)n_areas) + ", hour " + std::to_string((size_t)bad % H) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& V = ctx->hl1_area_var;
    ctx->has_hl1_area_var = false;
    HIP_TRY(ctx, V.out.grow(std::max<size_t>(n_out, 1)));
    if (n_out) HIP_TRY(ctx, hipMemcpy(V.out.get(), output_mw, sizeof(double) * n_out, hipMemcpyHostToDevice));
    if (load_mw) {
        HIP_TRY(ctx, V.load.grow(n_load));
        HIP_TRY(ctx, hipMemcpy(V.load.get(), load_mw, sizeof(double) * n_load, hipMemcpyHostToDevice));
    }
    V.n_areas = n_areas; V.n_weather = n_weather; V.n_res = n_resources; V.nhours = nhours; V.has_load = load_mw != nullptr;
    V.res_area.assign(resource_area, resource_area + n_resources);
    ctx->has_hl1_area_var = true;
    return RELMC_OK;
}

int32_t relmc_hl1_area_var(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                           const relmc_hl1_area_var_opts* opts, int32_t n_storage, const relmc_hl1_area_storage* storage,
                           relmc_hl1_storage_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_storage_year* storage_years_host,
                           int32_t* weather_host)
{
    const std::string who = "relmc_hl1_area_var: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_area) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_area_load has not been called");
    if (!ctx->has_hl1_area_var) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_area_var_load has not been called");
    auto& S = ctx->hl1_area;
    auto& V = ctx->hl1_area_var;
    if (S.n_areas != V.n_areas)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_areas of relmc_hl1_area_load " + std::to_string(S.n_areas) + " is not n_areas of relmc_hl1_area_var_load " +
                                            std::to_string(V.n_areas));
    if (S.nhours != V.nhours)
        return fail(ctx, RELMC_ERR_INVALID, who + "nhours of relmc_hl1_area_load " + std::to_string(S.nhours) + " is not nhours of relmc_hl1_area_var_load " +
                                            std::to_string(V.nhours));
    for (int r = 0; r < V.n_res; ++r)
        if (V.res_area[r] < 0 || V.res_area[r] >= S.n_areas)
            return fail(ctx, RELMC_ERR_INVALID, who + "resource " + std::to_string(r) + " is in area " + std::to_string(V.res_area[r]) + ", the model has " +
                                                std::to_string(S.n_areas) + " areas");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (!opts) return fail(ctx, RELMC_ERR_INVALID, who + "opts is null");
    relmc::AreaVarArgs A; std::memset(&A, 0, sizeof(A));
    if (const int rc = hl1_resource_scales(ctx, who, opts->resource_scale, V.n_res, A.rscale)) return rc;
    for (int r = 0; r < V.n_res; ++r) A.rarea[r] = V.res_area[r];
    for (int a = 0; a < RELMC_AREA_MAX; ++a) {
        const double sc = opts->load_scale[a], sh = opts->load_shift[a];
        const std::string la = who + "load_scale / load_shift of area " + std::to_string(a);
        if (!std::isfinite(sc) || !std::isfinite(sh)) return fail(ctx, RELMC_ERR_INVALID, la + " not finite");
        if (a >= S.n_areas && (sc != 1.0 || sh != 0.0)) return fail(ctx, RELMC_ERR_INVALID, la + " not 1 / 0 with n_areas " + std::to_string(S.n_areas));
        A.lscale[a] = sc; A.lshift[a] = sh;
    }
    if (opts->policy != RELMC_HL1_AREA_ISOLATED && opts->policy != RELMC_HL1_AREA_INTERCONNECTED)
        return fail(ctx, RELMC_ERR_INVALID, who + "policy " + std::to_string(opts->policy) + " not 0 or 1");
    if (opts->flow != RELMC_HL1_AREA_FLOW_REFERENCE && opts->flow != RELMC_HL1_AREA_FLOW_MAX_FLOW)
        return fail(ctx, RELMC_ERR_INVALID, who + "flow " + std::to_string(opts->flow) + " not 0 or 1");
    if (const int rc = hl1_pick_check(ctx, who, opts->pick, opts->reserved)) return rc;
    if (const int rc = hl1_storage_count_check(ctx, who, n_storage, storage)) return rc;
    for (int i = 0; i < n_storage; ++i) {
        const relmc_hl1_storage& v = storage[i].s;
        const std::string st = who + "storage " + std::to_string(i) + ": ";
        if (storage[i].area < 0 || storage[i].area >= S.n_areas)
            return fail(ctx, RELMC_ERR_INVALID, st + "area " + std::to_string(storage[i].area) + " not in 0.." + std::to_string(S.n_areas - 1));
        if (storage[i].reserved != 0) return fail(ctx, RELMC_ERR_INVALID, st + "reserved is not 0");
        if (const int rc = hl1_storage_check(ctx, st, v)) return rc;
        A.st[i] = v; A.sarea[i] = storage[i].area;
    }
    A.n_storage = n_storage; A.n_res = V.n_res; A.n_weather = V.n_weather; A.pick = opts->pick;
    A.out = V.out.get(); A.wload = V.has_load ? V.load.get() : nullptr;
    const int rows = S.n_areas + 1, slices = 2 * rows;
    std::memset(acc, 0, sizeof(*acc) * rows);
    if (n_chains == 0) return RELMC_OK;
    hl1_weather_fill(weather_host, seed, first_chain, n_chains, years_per_chain, V.n_weather, opts->pick);
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool inter = opts->policy == RELMC_HL1_AREA_INTERCONNECTED;
    const int nw = (S.ngen + 31) >> 5;
    const bool ties = inter && S.tie_outages && S.tie_fail;       // the tie-outage kernel: one more mask row
    const size_t lds = sizeof(double) * 64 * relmc::area_var_lds_rows(S.n_areas, inter, n_storage > 0) +
                       sizeof(uint32_t) * (nw + (ties ? 1 : 0)) * relmc::HL1_SEQ_WINDOW;
    const auto kernel = ties ? relmc::relmc_hl1_area_kernel<true, relmc::AreaVarArgs> : relmc::relmc_hl1_area_kernel<false, relmc::AreaVarArgs>;
    std::vector<double> stage, sum((size_t)slices * 6, 0.0);
    const int64_t total = n_chains * years_per_chain;
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)slices * years_per_chain);   // a chain counts its records of every slice
    const int rc = hl1_run_records(ctx, "relmc_hl1_area_var", V.rec, n_chains, per, years_per_chain, slices, sum.data(),
        [&](int64_t c0, int64_t nc, int64_t nrec) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nc), dim3(64), lds, ctx->stream, S.dcase.get(), ties ? S.dties.get() : nullptr, S.load.get(), seed,
                               first_chain + (uint64_t)c0, years_per_chain, start, opts->policy, opts->flow, nrec, A, V.rec.years.get());
        },
        [&](int64_t, int64_t, int64_t nrec) -> int {
            if (years_host || storage_years_host) {
                stage.resize((size_t)nrec * 3 * slices);
                HIP_TRY(ctx, hipMemcpyAsync(stage.data(), V.rec.years.get(), sizeof(double) * stage.size(), hipMemcpyDeviceToHost, ctx->stream));
            }
            return RELMC_OK;
        },
        [&](int64_t c0, int64_t, int64_t nrec) {                  // [slice][record] -> [record][row], one host array per record kind
            if (years_host) hl1_rows_to_host(stage, 1, rows, nrec, total, c0 * years_per_chain, years_host);
            if (storage_years_host)
                for (int64_t i = 0; i < nrec; ++i)
                    for (int r = 0; r < rows; ++r) {
                        relmc_hl1_storage_year& o = storage_years_host[(size_t)(c0 * years_per_chain + i) * rows + r];
                        const double* s = stage.data() + ((size_t)(rows + r) * nrec + i) * 3;
                        o.served_hours = s[0]; o.discharged_mwh = s[1]; o.charged_mwh = s[2];
                    }
        });
    if (rc) return rc;
    for (int r = 0; r < rows; ++r) hl1_storage_acc_fill(acc + r, total, sum.data() + (size_t)r * 6, sum.data() + (size_t)(rows + r) * 6);
    return RELMC_OK;
}

}  // extern "C"
