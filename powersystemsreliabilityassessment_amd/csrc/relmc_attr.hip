// relmc_attr.hip — loss attribution on the HL1 sequential chronology (relmc_hl1_attr_seq, contract in include/relmc.h): the loss hours and
// the unserved energy of relmc_hl1_seq's chains charged to the units that are DOWN in them, with the two exact counterfactuals (the
// steps and the energy that unit k, always UP, would have saved).
// A unit of its own, so that the code objects of relmc_seq.hip and the other tracks stay what they were; the kernels are
// relmc_hl1_attr_kernels.h's; the launches and the sums of the year records are relmc_hl1_host.h's hl1_run_records with one slice, and
// the chains' unit records of a launch are summed by relmc_hl1_attr_reduce_kernel, queued with the chain kernel.
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_hl1_attr_kernels.h"

using namespace relmc_host;

namespace {
// slices of relmc_hl1_attr_reduce_kernel's grid over n chain records: each workgroup 256 chains at a time, 64 slices at the most
int64_t attr_reduce_slices(int64_t n) { const int64_t b = (n + 255) / 256; return b < 64 ? b : 64; }
}  // namespace

extern "C" {

// Per chunk of chains one launch that walks every chain once and writes its year records ([chain][year][3]) and its unit records
// ([chain][unit][4]), then the two fixed-order reductions.  A chain counts years_per_chain + (4 * ngen + 2) / 3 records against the
// budget of a launch: its unit records are 4 * ngen doubles, a year record 3.  A chain's records never depend on the chunk it is in.
int32_t relmc_hl1_attr_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                           double scale, double shift, relmc_hl1_seq_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_attr_acc* unit_acc,
                           relmc_hl1_attr_unit* unit_host)
{
    const std::string who = "relmc_hl1_attr_seq: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_seq) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_seq_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (!unit_acc) return fail(ctx, RELMC_ERR_INVALID, who + "unit_acc is null");
    if (!std::isfinite(scale) || !std::isfinite(shift)) return fail(ctx, RELMC_ERR_INVALID, who + "scale / shift not finite");
    auto& S = ctx->hl1_seq;
    auto& A = ctx->hl1_attr;
    const int ngen = S.ngen;
    std::memset(acc, 0, sizeof(*acc));
    std::memset(unit_acc, 0, sizeof(*unit_acc) * ngen);
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain + (4 * (int64_t)ngen + 2) / 3);
    const int64_t slices_max = attr_reduce_slices(per);
    HIP_TRY(ctx, A.unit.grow((size_t)per * ngen * 4));
    HIP_TRY(ctx, A.upart.grow((size_t)slices_max * ngen * 8));
    std::vector<double> upart;
    double sum[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int rc = hl1_run_records(ctx, "relmc_hl1_attr_seq", A.rec, n_chains, per, years_per_chain, 1, sum,
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(relmc::relmc_hl1_attr_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, scale, shift, A.rec.years.get(), A.unit.get());
            hipLaunchKernelGGL(relmc::relmc_hl1_attr_reduce_kernel, dim3((unsigned)ngen, (unsigned)attr_reduce_slices(nc)), dim3(256), 0, ctx->stream,
                               (const double*)A.unit.get(), nc, ngen, A.upart.get());
        },
        [&](int64_t c0, int64_t nc, int64_t nrec) -> int {
            if (years_host)
                HIP_TRY(ctx, hipMemcpyAsync(years_host + c0 * years_per_chain, A.rec.years.get(), sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            if (unit_host)
                HIP_TRY(ctx, hipMemcpyAsync(unit_host + (size_t)c0 * ngen, A.unit.get(), sizeof(double) * 4 * (size_t)nc * ngen, hipMemcpyDeviceToHost, ctx->stream));
            upart.resize((size_t)attr_reduce_slices(nc) * ngen * 8);
            HIP_TRY(ctx, hipMemcpyAsync(upart.data(), A.upart.get(), sizeof(double) * upart.size(), hipMemcpyDeviceToHost, ctx->stream));
            return RELMC_OK;
        },
        [&](int64_t, int64_t nc, int64_t) {                  // unit_acc += the launch's partials, slice by slice (the order is part of the results)
            const int64_t slices = attr_reduce_slices(nc);
            for (int64_t b = 0; b < slices; ++b)
                for (int k = 0; k < ngen; ++k) {
                    const double* const p = upart.data() + ((size_t)b * ngen + k) * 8;
                    for (int j = 0; j < 4; ++j) { unit_acc[k].sum[j] += p[j]; unit_acc[k].sum2[j] += p[4 + j]; }
                }
        });
    if (rc) return rc;
    hl1_acc_fill(acc, n_chains * years_per_chain, sum);
    return RELMC_OK;
}

}  // extern "C"
