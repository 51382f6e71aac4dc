// relmc_multistate.hip — the HL1 sequential chronology with three-state units, UP / DERATED / DOWN (relmc_hl1_ms_load, relmc_hl1_ms_seq,
// contract in include/relmc.h).  A model slot and a unit of their own: no other HL1 call disturbs the model and relmc_seq.hip's code
// object stays what it was.  The two rows of year records, (lole, eue, lolf) and (derated_unit_h, down_unit_h, 0), are summed by
// relmc_hl1_reduce_kernel (hl1_reduce_queue, relmc_seq.hip), one row at a time; the second row leaves without its padding.
#include <algorithm>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "relmc_hl1_host.h"
#include "relmc_multistate_kernels.h"

using namespace relmc_host;

static_assert(sizeof(relmc_hl1_ms_unit) == 64, "relmc_hl1_ms_unit is 64 bytes");
static_assert(sizeof(relmc_hl1_ms_year) == 16, "relmc_hl1_ms_year is two doubles");
static_assert(sizeof(relmc_hl1_ms_acc) == 8 + 10 * sizeof(double), "relmc_hl1_ms_acc: years, the first row's six sums and the second row's four");

namespace {
const char* const kState[3] = {"UP", "DERATED", "DOWN"};
// the destinations of state s: first-listed, other
constexpr int kDest[3][2] = {{2, 1}, {0, 2}, {0, 1}};

// The checks of one unit's chain and its stationary start thresholds (the contract's expressions, in its order of operations).
// reach[s]: s can be reached from UP.  An empty string: accepted.
std::string ms_unit_chain(const relmc_hl1_ms_unit& u, bool reach[3], double* thr_down, double* thr_out)
{
    reach[0] = true; reach[1] = reach[2] = false;
    bool seen[3] = {false, false, false};
    for (;;) {                                               // states in the order they are reached; each is checked before its exits are used
        int s = -1;
        for (int t = 0; t < 3; ++t) if (reach[t] && !seen[t]) { s = t; break; }
        if (s < 0) break;
        seen[s] = true;
        if (!(u.first_p[s] >= 0.0 && u.first_p[s] <= 1.0)) return std::string("first_p of state ") + kState[s] + " not in [0, 1]";
        if (!(u.mean_h[s] > 0.0)) return std::string("mean_h of state ") + kState[s] + " not positive";
        if (u.first_p[s] > 0.0) reach[kDest[s][0]] = true;
        if (u.first_p[s] < 1.0) reach[kDest[s][1]] = true;
    }
    const double f0 = u.first_p[0], f1 = u.first_p[1], f2 = u.first_p[2];
    if (reach[1] && reach[2]) {
        if (!(f1 > 0.0 || f2 > 0.0)) return "DERATED and DOWN cannot return to UP";
        const double nu0 = f2 + f1 * (1.0 - f2), nu1 = (1.0 - f2) + f2 * (1.0 - f0), nu2 = (1.0 - f1) + f1 * f0;
        const double w0 = nu0 * u.mean_h[0], w1 = nu1 * u.mean_h[1], w2 = nu2 * u.mean_h[2], sum = (w0 + w1) + w2;
        const double pi2 = w2 / sum, pi1 = w1 / sum;
        *thr_down = pi2; *thr_out = pi2 + pi1;
    } else if (reach[2]) {                                   // UP <-> DOWN: hl1_units_fill's q
        *thr_down = u.mean_h[2] / (u.mean_h[0] + u.mean_h[2]); *thr_out = *thr_down;
    } else {                                                 // UP <-> DERATED
        *thr_down = 0.0; *thr_out = u.mean_h[1] / (u.mean_h[0] + u.mean_h[1]);
    }
    return std::string();
}
}  // namespace

extern "C" {

int32_t relmc_hl1_ms_load(relmc_ctx* ctx, int32_t ngen, const relmc_hl1_ms_unit* units, int32_t nhours, const double* load_mw)
{
    const std::string who = "relmc_hl1_ms_load: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!units || !load_mw || ngen < 1 || nhours < 1) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    if (ngen > NCOMPMAX) return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "more than 128 units");
    // the kernel counts a lane's DERATED / DOWN (unit, step) pairs of a year in 32 bits: at most 128 * (nhours / 64 + 2) of them
    if (nhours > RELMC_HL1_MS_MAX_HOURS) return fail(ctx, RELMC_ERR_UNSUPPORTED, who + "more than 2^30 hours in the load curve");
    Hl1MsCase h; std::memset(&h, 0, sizeof(h));
    h.ngen = ngen; h.nhours = nhours;
    for (int g = 0; g < ngen; ++g) {
        const relmc_hl1_ms_unit& u = units[g];
        const std::string unit = " of unit " + std::to_string(g);
        if (!std::isfinite(u.capacity_mw)) return fail(ctx, RELMC_ERR_INVALID, who + "capacity" + unit + " not finite");
        if (!std::isfinite(u.derated_mw)) return fail(ctx, RELMC_ERR_INVALID, who + "derated_mw" + unit + " not finite");
        for (int s = 0; s < 3; ++s)
            if (!std::isfinite(u.mean_h[s]) || !std::isfinite(u.first_p[s]))
                return fail(ctx, RELMC_ERR_INVALID, who + "mean_h / first_p of state " + kState[s] + unit + " not finite");
        if (!(u.derated_mw >= 0.0 && u.derated_mw <= u.capacity_mw)) return fail(ctx, RELMC_ERR_INVALID, who + "derated_mw" + unit + " not in [0, capacity_mw]");
        bool reach[3];
        if (const std::string bad = ms_unit_chain(u, reach, &h.thr_down[g], &h.thr_out[g]); !bad.empty())
            return fail(ctx, RELMC_ERR_INVALID, who + bad + " (unit " + std::to_string(g) + ")");
        h.cap[g][0] = u.capacity_mw; h.cap[g][1] = u.derated_mw;
        for (int s = 0; s < 3; ++s) {                        // a state that is never entered is never read: neutral values
            h.mean[s][g] = reach[s] ? u.mean_h[s] : 1.0;
            h.first_p[s][g] = reach[s] ? u.first_p[s] : 1.0;
        }
    }
    if (const int64_t bad = first_non_finite(load_mw, nhours); bad >= 0)
        return fail(ctx, RELMC_ERR_INVALID, who + "load of hour " + std::to_string(bad) + " not finite");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_ms;
    ctx->has_hl1_ms = false;
    HIP_TRY(ctx, S.dcase.grow(1));
    HIP_TRY(ctx, S.load.grow((size_t)nhours));
    HIP_TRY(ctx, hipMemcpy(S.dcase.get(), &h, sizeof(h), hipMemcpyHostToDevice));
    HIP_TRY(ctx, hipMemcpy(S.load.get(), load_mw, sizeof(double) * nhours, hipMemcpyHostToDevice));
    S.ngen = ngen; S.nhours = nhours; ctx->has_hl1_ms = true;
    return RELMC_OK;
}

int32_t relmc_hl1_ms_seq(relmc_ctx* ctx, uint64_t seed, uint64_t first_chain, int64_t n_chains, int32_t years_per_chain, int32_t start,
                         relmc_hl1_ms_acc* acc, relmc_hl1_seq_year* years_host, relmc_hl1_ms_year* state_years_host)
{
    const std::string who = "relmc_hl1_ms_seq: ";
    if (!ctx) return RELMC_ERR_INVALID;
    if (!ctx->has_hl1_ms) return fail(ctx, RELMC_ERR_NO_CASE, who + "relmc_hl1_ms_load has not been called");
    if (!hl1_chain_args_ok(acc, n_chains, years_per_chain, start)) return fail(ctx, RELMC_ERR_INVALID, who + "bad arguments");
    std::memset(acc, 0, sizeof(*acc));
    if (n_chains == 0) return RELMC_OK;
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    auto& S = ctx->hl1_ms;
    std::vector<double> row1;
    double sum[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int64_t per = hl1_chunk_items(n_chains, kHl1RecordBudget, (int64_t)years_per_chain * 2);             // a chain counts its records of both rows
    const int rc = hl1_run_records(ctx, "relmc_hl1_ms_seq", S.rec, n_chains, per, years_per_chain, 2, sum,
        [&](int64_t c0, int64_t nc, int64_t) {
            hipLaunchKernelGGL(relmc_hl1_ms_kernel, dim3((unsigned)((nc + 3) / 4)), dim3(256), 0, ctx->stream, S.dcase.get(), S.load.get(), seed,
                               first_chain + (uint64_t)c0, nc, years_per_chain, start, S.rec.years.get());
        },
        [&](int64_t c0, int64_t, int64_t nrec) -> int {
            if (years_host)
                HIP_TRY(ctx, hipMemcpyAsync(years_host + c0 * years_per_chain, S.rec.years.get(), sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            if (state_years_host) {
                row1.resize((size_t)nrec * 3);
                HIP_TRY(ctx, hipMemcpyAsync(row1.data(), S.rec.years.get() + (size_t)nrec * 3, sizeof(double) * 3 * nrec, hipMemcpyDeviceToHost, ctx->stream));
            }
            return RELMC_OK;
        },
        [&](int64_t c0, int64_t, int64_t nrec) {             // the second row leaves without its padding
            if (!state_years_host) return;
            relmc_hl1_ms_year* const dst = state_years_host + c0 * years_per_chain;
            for (int64_t i = 0; i < nrec; ++i) { dst[i].derated_unit_h = row1[(size_t)3 * i]; dst[i].down_unit_h = row1[(size_t)3 * i + 1]; }
        });
    if (rc) return rc;
    acc->years = n_chains * years_per_chain;
    acc->sum_lole = sum[0]; acc->sum_eue = sum[1]; acc->sum_lolf = sum[2]; acc->sum_lole2 = sum[3]; acc->sum_eue2 = sum[4]; acc->sum_lolf2 = sum[5];
    acc->sum_derated = sum[6]; acc->sum_down = sum[7]; acc->sum_derated2 = sum[9]; acc->sum_down2 = sum[10];
    return RELMC_OK;
}

}  // extern "C"
