// relmc_maint.hip — planned maintenance on the HL1 sequential chronology (relmc_hl1_maint_load, relmc_hl1_maint_seq, contract in
// include/relmc.h): the fleet of relmc_hl1_seq_load under up to 8 maintenance schedules, all compared on one fleet history.
// A unit of its own, so that the code objects of relmc_seq.hip and the other tracks stay what they were; the kernel is the maintenance
// model of relmc_hl1_chain_kernels.h's template, of which this unit holds the four instantiations it launches and nothing else; the
// launches and the sums are relmc_hl1_host.h's hl1_run_records with one slice per schedule, the slices summed by
// relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip).
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_hl1_chain_kernels.h"

using namespace relmc_host;

namespace {
// The four instantiations of relmc_hl1_chain_kernels.h's template that this unit launches (NS = the schedules a walk compares)
template <int NS>
constexpr auto relmc_hl1_maint_kernel = relmc::relmc_hl1_chain_kernel<relmc::HL1_CHAIN_MAINT, NS, double, double, int32_t, const uint32_t* __restrict__, double* __restrict__>;

// schedules the kernel instantiation for n_schedules walks (relmc_hl1_maint_kernel<1, 2, 4, 8>): the table holds that many
int maint_width(int n_schedules) { return n_schedules <= 1 ? 1 : n_schedules <= 2 ? 2 : n_schedules <= 4 ? 4 : 8; }
}  // namespace

extern "C" {

int32_t relmc_hl1_maint_load(relmc_ctx* ctx, int32_t n_schedules, int64_t n_windows, const relmc_hl1_maint_window* windows)
{
    const std::string who = "relmc_hl1_maint_load: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_seq_load has not been called");
    if (n_schedules < 1 || n_schedules > RELMC_HL1_MAINT_MAX_SCHEDULES)
        return fail(ctx, RELMC_ERR_INVALID, who + "n_schedules " + std::to_string(n_schedules) + " not in 1.." + std::to_string(RELMC_HL1_MAINT_MAX_SCHEDULES));
    if (n_windows < 0) return fail(ctx, RELMC_ERR_INVALID, who + "n_windows " + std::to_string(n_windows) + " is negative");
    if (n_windows > 0 && !windows) return fail(ctx, RELMC_ERR_INVALID, who + "n_windows > 0 without windows");
    const int ngen = ctx->hl1_seq.ngen, H = ctx->hl1_seq.nhours;
    for (int64_t i = 0; i < n_windows; ++i) {
        const relmc_hl1_maint_window& w = windows[i];
        const std::string win = who + "window " + std::to_string(i) + ": ";
        if (w.schedule < 0 || w.schedule >= n_schedules)
            return fail(ctx, RELMC_ERR_INVALID, win + "schedule " + std::to_string(w.schedule) + " not in 0.." + std::to_string(n_schedules - 1));
        if (w.unit < 0 || w.unit >= ngen) return fail(ctx, RELMC_ERR_INVALID, win + "unit " + std::to_string(w.unit) + " not in 0.." + std::to_string(ngen - 1));
        if (w.start_hour < 0 || w.start_hour >= H)
            return fail(ctx, RELMC_ERR_INVALID, win + "start_hour " + std::to_string(w.start_hour) + " not in 0.." + std::to_string(H - 1));
        if (w.hours < 1 || w.hours > H) return fail(ctx, RELMC_ERR_INVALID, win + "hours " + std::to_string(w.hours) + " not in 1.." + std::to_string(H));
    }
    // tab[schedule][hour][4]; a window is the hours start_hour .. start_hour + hours - 1, those at or past H taken from hour 0 on
    const int width = maint_width(n_schedules);
    std::vector<uint32_t> tab((size_t)width * (size_t)H * 4, 0u);
    for (int64_t i = 0; i < n_windows; ++i) {
        const relmc_hl1_maint_window& w = windows[i];
        uint32_t* const row = tab.data() + (size_t)w.schedule * (size_t)H * 4 + (size_t)(w.unit >> 5);
        const uint32_t bit = 1u << (w.unit & 31);
        const int64_t end = (int64_t)w.start_hour + w.hours, first_end = end < H ? end : H;
        for (int64_t h = w.start_hour; h < first_end; ++h) row[(size_t)h * 4] |= bit;
        for (int64_t h = 0; h < end - H; ++h) row[(size_t)h * 4] |= bit;          // end - H <= start_hour: hours <= H
    }
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& M = ctx->hl1_maint;
    ctx->has_hl1_maint = false;
    HIP_TRY(ctx, M.tab.grow(tab.size()));
    HIP_TRY(ctx, hipMemcpy(M.tab.get(), tab.data(), sizeof(uint32_t) * tab.size(), hipMemcpyHostToDevice));
    M.n_schedules = n_schedules; M.ngen = ngen; M.nhours = H;
    ctx->has_hl1_maint = true;
    return RELMC_OK;
}

// Per chunk of chains one launch that walks every chain once and writes the year records of all schedules ([schedule][chain][year][3]),
// then relmc_hl1_reduce_kernel over each schedule's slice.  A chunk holds at most ~4M year records over all schedules; a chain's
// records never depend on the chunk it is in.
int32_t relmc_hl1_maint_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                            double scale, double shift, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host)
{
    const std::string who = "relmc_hl1_maint_seq: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_seq_load has not been called");
    if (!ctx->has_hl1_maint) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_maint_load has not been called");
    auto& S = ctx->hl1_seq;
    auto& M = ctx->hl1_maint;
    if (M.ngen != S.ngen)
        return fail(ctx, RELMC_ERR_INVALID, who + "ngen of relmc_hl1_maint_load " + std::to_string(M.ngen) + " is not ngen of relmc_hl1_seq_load " + std::to_string(S.ngen));
    if (M.nhours != S.nhours)
        return fail(ctx, RELMC_ERR_INVALID, who + "nhours of relmc_hl1_maint_load " + std::to_string(M.nhours) + " is not nhours of relmc_hl1_seq_load " + std::to_string(S.nhours));
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (!std::isfinite(scale) || !std::isfinite(shift)) return fail(ctx, RELMC_ERR_INVALID, who + "scale / shift not finite");
    const int ns = M.n_schedules;
    const int64_t total = n_chains * years_per_chain;
    std::memset(acc, 0, sizeof(*acc) * ns);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int width = maint_width(ns);
    const auto kernel = width == 1 ? relmc_hl1_maint_kernel<1> : width == 2 ? relmc_hl1_maint_kernel<2>
                      : width == 4 ? relmc_hl1_maint_kernel<4> : relmc_hl1_maint_kernel<8>;
    std::vector<double> sum((size_t)6 * ns, 0.0);
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * ns);      // a chain counts its records of all schedules
    const int rc = hl1_run_records(ctx, "relmc_hl1_maint_seq", M.rec, n_chains, per, years_per_chain, ns, sum.data(),
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, scale, shift, ns, (const uint32_t*)M.tab.get(), M.rec.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) -> int {
            if (years_host)
                for (int j = 0; j < ns; ++j)
                    HIP_TRY(ctx, hipMemcpyAsync(years_host + (size_t)j * total + c0 * years_per_chain, M.rec.years.get() + (size_t)j * nrec * 3,
                                                sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        hl1_no_host_step);
    if (rc) return rc;
    for (int j = 0; j < ns; ++j) hl1_acc_fill(acc + j, total, sum.data() + (size_t)6 * j);
    return RELMC_OK;
}

}  // extern "C"
