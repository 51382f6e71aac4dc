// relmc_hl1_host.h — host code the HL1 record models share: the unit and argument checks, the chunk rule, and the one loop that launches
// a model chunk by chunk and sums its year records (hl1_run_records).  Host only.  `who` is the calling function's name, for the message.
// The buffer pair of a model, Hl1Records, is in relmc_ctx.h: the context holds one per model by value.
#pragma once
#include <algorithm>

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

}  // namespace relmc_host
