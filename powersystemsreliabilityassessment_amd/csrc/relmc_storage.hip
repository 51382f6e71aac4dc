// relmc_storage.hip — energy storage with a state of charge on the HL1 sequential chronology (relmc_hl1_seq_storage, contract in
// include/relmc.h): the model of relmc_hl1_seq_load (relmc_seq.hip) at one load level, with up to RELMC_HL1_MAX_STORAGE storages given in
// the call.  A unit of its own, so that relmc_seq.hip's code object stays what it was.  The storage checks and the accumulator fill are
// relmc_hl1_host.h's, the kernel the storage track of relmc_hl1_storage_kernels.h.  The two rows of year records, (lole, eue, lolf)
// and (served_hours, discharged_mwh, charged_mwh), are summed by relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row at a time.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_hl1_storage_kernels.h"

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
    if (const int rc = hl1_storage_count_check(ctx, who, n_storage, storage)) return rc;
    Hl1StorageArgs A; std::memset(&A, 0, sizeof(A));
    A.scale = scale; A.shift = shift; A.n_storage = n_storage;
    for (int i = 0; i < n_storage; ++i) {
        const relmc_hl1_storage& v = storage[i];
        const std::string st = who + "storage " + std::to_string(i) + ": ";
        if (const int rc = hl1_storage_check(ctx, st, v)) return rc;
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
            hipLaunchKernelGGL(relmc_hl1_storage_track_kernel<HL1_TRACK_STORAGE>, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, A, X.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) { return hl1_two_row_copies(ctx, X.years.get(), c0 * years_per_chain, nrec, years_host, storage_years_host); },
        hl1_no_host_step);
    if (rc) return rc;
    hl1_storage_acc_fill(acc, n_chains * years_per_chain, sum, sum + 6);
    return RELMC_OK;
}

}  // extern "C"
