// relmc_area_sweep.hip — sweep of the HL1 multi-area chronology (relmc_hl1_area_sweep, contract in include/relmc.h): the model of
// relmc_hl1_area_load / relmc_hl1_area_tie_outages (relmc_area.hip) against up to 8 levels of load, tie capacity and fleet in one walk of
// every chain.  A unit of its own, so that relmc_area.hip's code object stays what it was.  The per-level, per-row year records are
// summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one slice at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_area_sweep_kernels.h"

using namespace relmc_host;

static_assert(relmc::AREA_SWEEP_MAX_LEVELS == RELMC_HL1_AREA_SWEEP_MAX_LEVELS, "relmc_dev.h and include/relmc.h disagree on the level limit");
static_assert(sizeof(relmc_hl1_area_level) == 144, "relmc_hl1_area_level is 144 bytes");

extern "C" {

int32_t relmc_hl1_area_sweep(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                             int32_t flow, int32_t n_levels, const relmc_hl1_area_level* levels, const uint32_t* withheld,
                             const uint8_t* tie_scaled, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host)
{
    const std::string who = "relmc_hl1_area_sweep: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_area) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_area_load has not been called");
    if (!levels || !hl1_chain_args_ok(acc, n_chains, years_per_chain, start) ||
        (flow != RELMC_HL1_AREA_FLOW_REFERENCE && flow != RELMC_HL1_AREA_FLOW_MAX_FLOW))
        return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (n_levels < 1 || n_levels > RELMC_HL1_AREA_SWEEP_MAX_LEVELS)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_levels " + std::to_string(n_levels) + " not in 1.." + std::to_string(RELMC_HL1_AREA_SWEEP_MAX_LEVELS));
    auto& S = ctx->hl1_area;
    const int na = S.n_areas, rows = na + 1, nt = (int)S.tie_cap.size();
    relmc::AreaSweepTab tab; std::memset(&tab, 0, sizeof(tab));
    tab.n_levels = n_levels;
    for (int j = 0; j < n_levels; ++j) {
        const relmc_hl1_area_level& v = levels[j];
        const std::string lvl = who + "level " + std::to_string(j);
        relmc::AreaSweepLevelTab& t = tab.lv[j];
        for (int a = 0; a < na; ++a) {
            if (!std::isfinite(v.load_scale[a]) || !std::isfinite(v.load_shift[a]))
                return fail(ctx, RELMC_ERR_INVALID, lvl + ": load scale / shift of area " + std::to_string(a) + " not finite");
            t.scale[a] = v.load_scale[a]; t.shift[a] = v.load_shift[a];
        }
        if (!(std::isfinite(v.tie_scale) && v.tie_scale >= 0.0)) return fail(ctx, RELMC_ERR_INVALID, lvl + ": tie_scale not finite and >= 0");
        if (v.fleet != 0 && v.fleet != 1) return fail(ctx, RELMC_ERR_INVALID, lvl + ": fleet " + std::to_string(v.fleet) + " is not 0 or 1");
        if (v.reserved != 0) return fail(ctx, RELMC_ERR_INVALID, lvl + ": reserved must be 0");
        if (v.fleet == 1 && !withheld) return fail(ctx, RELMC_ERR_INVALID, lvl + ": fleet 1 without a withheld mask");
        if (v.fleet == 1) tab.fleet1 |= 1u << j;
        for (int l = 0; l < nt; ++l) {                       // relmc_hl1_area_load's T on the level's capacities: parallel ties summed in tie order
            const bool scaled = !tie_scaled || tie_scaled[l] != 0;
            const double c = scaled ? v.tie_scale * S.tie_cap[l] : S.tie_cap[l];
            if (!std::isfinite(c)) return fail(ctx, RELMC_ERR_INVALID, lvl + ": scaled capacity of tie " + std::to_string(l) + " not finite");
            const int p = S.tie_from[l], q = S.tie_to[l];
            t.tie[p * na + q] += c;
            t.tie[q * na + p] += c;
            if (l < relmc::AREA_TIE_MAX) t.cap[l] = c;       // read with outage data only, which has at most that many ties
            if (c > 0.0) tab.solve |= 1u << j;
        }
    }
    if (withheld) {
        for (int k = S.ngen; k < 128; ++k)
            if ((withheld[k >> 5] >> (k & 31)) & 1u)
                return fail(ctx, RELMC_ERR_INVALID, who + "withheld bit " + std::to_string(k) + " at or above ngen = " + std::to_string(S.ngen));
        std::memcpy(tab.withheld, withheld, sizeof(tab.withheld));
    }
    const int64_t total = n_chains * years_per_chain;
    const int slices = n_levels * rows;                      // record slices of a launch: [level][row]
    std::memset(acc, 0, sizeof(*acc) * slices);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, S.sweep_tab.grow(1));
    HIP_TRY(ctx, hipMemcpy(S.sweep_tab.get(), &tab, sizeof(tab), hipMemcpyHostToDevice));
    const int nw = (S.ngen + 31) >> 5;
    const bool ties = S.tie_outages && S.tie_fail;          // relmc_hl1_area's rule under INTERCONNECTED: the tie cursors, one more mask row
    const size_t lds = sizeof(double) * 64 * ((size_t)n_levels * rows + na + na * na) +
                       sizeof(uint32_t) * (nw + (ties ? 1 : 0)) * relmc::HL1_SEQ_WINDOW;
    const auto kernel = ties ? relmc::relmc_hl1_area_sweep_kernel<true> : relmc::relmc_hl1_area_sweep_kernel<false>;
    if (lds > 64 * 1024)                                     // 8 levels x 8 areas: 83 KB of the CU's 160 KB
        HIP_TRY(ctx, hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
    std::vector<double> stage, sum((size_t)slices * 6, 0.0);
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * slices);        // a chain counts its records of all levels and rows
    const int rc = hl1_run_records(ctx, "relmc_hl1_area_sweep", S.sweep_rec, n_chains, per, years_per_chain, slices, sum.data(),
        [&](int64_t c0, int64_t nc, int64_t nrec) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nc), dim3(64), lds, ctx->stream, S.dcase.get(), ties ? S.dties.get() : nullptr, S.sweep_tab.get(),
                               S.load.get(), seed, first_chain + (uint64_t)c0, years_per_chain, start, flow, nrec, S.sweep_rec.years.get());
        },
        [&](int64_t, int64_t, int64_t nrec) -> int {
            if (years_host) {
                stage.resize((size_t)nrec * 3 * slices);
                HIP_TRY(ctx, hipMemcpyAsync(stage.data(), S.sweep_rec.years.get(), sizeof(double) * stage.size(), hipMemcpyDeviceToHost, ctx->stream));
            }
            return RELMC_OK;
        },
        [&](int64_t c0, int64_t, int64_t nrec) {                  // [level][row][record] -> [level][record][row]
            if (years_host) hl1_rows_to_host(stage, n_levels, rows, nrec, total, c0 * years_per_chain, years_host);
        });
    if (rc) return rc;
    for (int s = 0; s < slices; ++s) hl1_acc_fill(acc + s, total, sum.data() + (size_t)s * 6);
    return RELMC_OK;
}

}  // extern "C"
