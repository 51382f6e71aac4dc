// relmc_area.hip — the HL1 multi-area chronology with tie-line transfers (GeneratingAdequacy/AdequacyAssessmentII.jl:73-250; contract in
// include/relmc.h).  The per-row year records are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row slice at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_area_kernels.h"

using namespace relmc_host;

static_assert(relmc::AREA_MAX == RELMC_AREA_MAX, "relmc_dev.h and include/relmc.h disagree on the area limit");
static_assert(relmc::AREA_TIE_MAX == RELMC_HL1_TIE_MAX && relmc::AREA_TIE_DRAW_BASE == RELMC_HL1_TIE_DRAW_BASE,
              "relmc_dev.h and include/relmc.h disagree on the tie limits");
static_assert(relmc::AREA_TIE_DRAW_BASE >= relmc::NCOMPMAX, "tie draws must not share a component index with a unit");

extern "C" {

int32_t relmc_hl1_area_load(relmc_ctx* ctx, int32_t n_areas, const int32_t* units_per_area, const double* capacity_mw,
                            const double* mttf_h, const double* mttr_h, int32_t nhours, const double* hourly_load_mw,
                            int32_t n_ties, const int32_t* tie_from, const int32_t* tie_to, const double* tie_capacity_mw)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!units_per_area || !capacity_mw || !mttf_h || !mttr_h || !hourly_load_mw || n_areas < 1 || nhours < 1 || n_ties < 0 ||
        (n_ties > 0 && (!tie_from || !tie_to || !tie_capacity_mw)))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_load: bad arguments");
    if (n_areas > RELMC_AREA_MAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_area_load: more than 8 areas");
    relmc::AreaCase A; std::memset(&A, 0, sizeof(A));
    int64_t ngen = 0;
    for (int a = 0; a < n_areas; ++a) {
        if (units_per_area[a] < 1) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_load: area " + std::to_string(a) + " has no unit");
        A.lo[a] = (int32_t)std::min<int64_t>(ngen, NCOMPMAX);
        ngen += units_per_area[a];
    }
    if (ngen > NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, "relmc_hl1_area_load: more than 128 units");
    A.lo[n_areas] = (int32_t)ngen;
    A.ngen = (int32_t)ngen; A.nhours = nhours; A.n_areas = n_areas;
    if (const int rc = hl1_units_fill(ctx, "relmc_hl1_area_load", (int)ngen, capacity_mw, mttf_h, mttr_h, A.cap, A.mttf, A.mttr, A.q)) return rc;
    if (const int64_t bad = first_non_finite(hourly_load_mw, (int64_t)n_areas * nhours); bad >= 0)
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_load: load of area " + std::to_string(bad / nhours) + " hour " + std::to_string(bad % nhours) +
                                            " not finite");
    for (int l = 0; l < n_ties; ++l) {
        const int i = tie_from[l], j = tie_to[l];
        if (i < 0 || i >= n_areas || j < 0 || j >= n_areas || i == j)
            return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_load: tie " + std::to_string(l) + " has a bad endpoint");
        if (!(std::isfinite(tie_capacity_mw[l]) && tie_capacity_mw[l] >= 0.0))
            return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_load: capacity of tie " + std::to_string(l) + " not finite and >= 0");
        A.tie[i * n_areas + j] += tie_capacity_mw[l];              // System(areas, lines), :50-59: parallel ties summed in tie order
        A.tie[j * n_areas + i] += tie_capacity_mw[l];
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_area;
    ctx->has_hl1_area = false;
    HIP_TRY(ctx, S.dcase.grow(1));
    HIP_TRY(ctx, S.load.grow((size_t)n_areas * nhours));
    HIP_TRY(ctx, hipMemcpy(S.dcase.get(), &A, sizeof(A), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.load.get(), hourly_load_mw, sizeof(double) * n_areas * nhours, hipMemcpyHostToDevice));
    S.ngen = (int)ngen; S.nhours = nhours; S.n_areas = n_areas; ctx->has_hl1_area = true;
    S.tie_from.assign(tie_from, tie_from + n_ties); S.tie_to.assign(tie_to, tie_to + n_ties);
    S.tie_cap.assign(tie_capacity_mw, tie_capacity_mw + n_ties);
    S.tie_outages = S.tie_fail = false;                            // a new model has no outage data
    return RELMC_OK;
}

int32_t relmc_hl1_area_tie_outages(relmc_ctx* ctx, int32_t n_ties, const double* tie_mttf_h, const double* tie_mttr_h)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_area) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_area_tie_outages: relmc_hl1_area_load has not been called");
    auto& S = ctx->hl1_area;
    if (n_ties < 0 || (!tie_mttf_h) != (!tie_mttr_h)) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_tie_outages: bad arguments");
    if (n_ties == 0 || !tie_mttf_h) { S.tie_outages = S.tie_fail = false; return RELMC_OK; }
    if (n_ties > RELMC_HL1_TIE_MAX) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_tie_outages: more than 32 ties");
    if ((size_t)n_ties != S.tie_cap.size())
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_tie_outages: " + std::to_string(n_ties) + " ties, the loaded model has " +
                                            std::to_string(S.tie_cap.size()));
    relmc::AreaTies TL; std::memset(&TL, 0, sizeof(TL));
    TL.n_ties = n_ties;
    bool any = false;
    for (int t = 0; t < n_ties; ++t) {
        const double f = tie_mttf_h[t];
        if (!(f > 0.0)) return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_tie_outages: MTTF of tie " + std::to_string(t) + " not > 0 or +inf");
        TL.from[t] = S.tie_from[t]; TL.to[t] = S.tie_to[t]; TL.cap[t] = S.tie_cap[t];
        TL.mttf[t] = f; TL.mttr[t] = 1.0; TL.q[t] = 0.0;
        if (std::isinf(f)) continue;                               // never fails: mttr is not read
        const double r = tie_mttr_h[t];
        if (!(std::isfinite(r) && r > 0.0))
            return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area_tie_outages: MTTR of tie " + std::to_string(t) + " not finite and positive");
        TL.mttr[t] = r; TL.q[t] = r / (f + r);
        any = true;
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    HIP_TRY(ctx, S.dties.grow(1));
    HIP_TRY(ctx, hipMemcpy(S.dties.get(), &TL, sizeof(TL), hipMemcpyHostToDevice));
    S.tie_outages = true; S.tie_fail = any;
    return RELMC_OK;
}

int32_t relmc_hl1_area(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                       int32_t policy, int32_t flow, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host)
{
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_area) return fail(ctx, RELMC_ERR_NO_CASE, "relmc_hl1_area: relmc_hl1_area_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start) ||
        (policy != RELMC_HL1_AREA_ISOLATED && policy != RELMC_HL1_AREA_INTERCONNECTED) ||
        (flow != RELMC_HL1_AREA_FLOW_REFERENCE && flow != RELMC_HL1_AREA_FLOW_MAX_FLOW))
        return fail(ctx, RELMC_ERR_INVALID, "relmc_hl1_area: bad arguments");
    auto& S = ctx->hl1_area;
    const int rows = S.n_areas + 1;
    std::memset(acc, 0, sizeof(*acc) * rows);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const bool inter = policy == RELMC_HL1_AREA_INTERCONNECTED;
    const int nw = (S.ngen + 31) >> 5;
    const bool ties = inter && S.tie_outages && S.tie_fail;       // the tie-outage kernel: one more mask row
    const size_t lds = sizeof(double) * 64 * (2 * S.n_areas + 1 + (inter ? S.n_areas * S.n_areas : 0)) +
                       sizeof(uint32_t) * (nw + (ties ? 1 : 0)) * relmc::HL1_SEQ_WINDOW;
    const auto kernel = ties ? relmc::relmc_hl1_area_kernel<true> : relmc::relmc_hl1_area_kernel<false>;
    std::vector<double> stage, sum((size_t)rows * 6, 0.0);
    // records [row][chain * years + year][3], rows one slice apart.  A chain counts the year records of ONE row here (the other models
    // count every slice): a launch holds ~4M year records x rows, as it has since the model was added
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, years_per_chain);
    const int rc = hl1_run_records(ctx, "relmc_hl1_area", S.rec, n_chains, per, years_per_chain, rows, sum.data(),
        [&](int64_t c0, int64_t nc, int64_t nrec) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)nc), dim3(64), lds, ctx->stream, S.dcase.get(), ties ? S.dties.get() : nullptr, S.load.get(), seed,
                               first_chain + (uint64_t)c0, years_per_chain, start, policy, flow, nrec, S.rec.years.get());
        },
        [&](int64_t, int64_t, int64_t nrec) -> int {
            if (years_host) {
                stage.resize((size_t)nrec * 3 * rows);
                HIP_TRY(ctx, hipMemcpyAsync(stage.data(), S.rec.years.get(), sizeof(double) * stage.size(), hipMemcpyDeviceToHost, ctx->stream));
            }
            return RELMC_OK;
        },
        [&](int64_t c0, int64_t, int64_t nrec) {                  // [row][record] -> [record][row]
            if (years_host) hl1_rows_to_host(stage, 1, rows, nrec, n_chains * years_per_chain, c0 * years_per_chain, years_host);
        });
    if (rc) return rc;
    for (int r = 0; r < rows; ++r) hl1_acc_fill(acc + r, n_chains * years_per_chain, sum.data() + (size_t)r * 6);
    return RELMC_OK;
}

}  // extern "C"
